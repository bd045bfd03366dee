// One iteration of the ActionBench ICP (actionbench/icp.py:86-106) without an autograd graph: am_icp_step of include/actionmesh_amd.h,
// whose comment is the contract - every operation below is written in the order it gives, and this file is built without contraction.
// The Chamfer loss's gradient with respect to the 12 parameters of a candidate is a function of 13 sums over the matched pairs, and a
// lane of the search holds exactly one matched pair in registers when its loop ends: the sums are formed there.
//
//   icp_pairs_kernel   grid = (query blocks of direction 0 + query blocks of direction 1, 1, batch), 256 threads, one query each.
//                      The search is am_points.h's staged scan, the one nn_search_kernel<float, 1> runs (am_pointcloud.hip).
//                      Direction 0: queries x_i, points y_j.  Direction 1: queries y_j, points x_i, transformed while staged.
//                      Lane 0 of the workgroup forms R in fp64 first (a few hundred fp64 operations beside 256 x n_points distances).
//                      Epilogue: 13 fp64 terms per lane -> __shfl_down tree over the 64 lanes -> the 4 waves through LDS -> one
//                      (13) partial per workgroup in the workspace.  No float atomics.
//   icp_update_kernel  ONE workgroup: the partials summed in workgroup order, then one candidate per lane: loss, chain rule, Adam;
//                      then the smallest loss of the batch against the stored best.
#include "am_points.h"

namespace {

constexpr int ICP_THREADS = NN_THREADS;
constexpr int ICP_WAVES = ICP_THREADS / 64;
constexpr int ICP_TERMS = 13;

// step 1's results: what the points need (R, with T and s beside it) and what the backward pass needs again
struct IcpXf { float R[9], T[3], s[3]; };
struct IcpFrame { double a1[3], a2[3], b1[3], b2[3], n1, n2, d; };

__device__ __forceinline__ double icp_dot(const double* u, const double* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }
__device__ __forceinline__ void icp_cross(const double* u, const double* v, double* o) {
  o[0] = u[1] * v[2] - u[2] * v[1];
  o[1] = u[2] * v[0] - u[0] * v[2];
  o[2] = u[0] * v[1] - u[1] * v[0];
}

// step 1: params (12) and rot_init (9) of one candidate -> R = fl32(rot_init . G(d6)), T, s; the Gram-Schmidt quantities in `fr`
__device__ __forceinline__ void icp_rotation(const float* __restrict__ prm, const float* __restrict__ ri, IcpXf& xf, IcpFrame& fr) {
#pragma clang fp contract(off)
  for (int j = 0; j < 3; ++j) {
    fr.a1[j] = (double)prm[3 + j];
    fr.a2[j] = (double)prm[6 + j];
    xf.T[j] = prm[j];
    xf.s[j] = prm[9 + j];
  }
  const double l1 = sqrt(icp_dot(fr.a1, fr.a1));
  fr.n1 = l1 < 1e-12 ? 1e-12 : l1;
  for (int j = 0; j < 3; ++j) fr.b1[j] = fr.a1[j] / fr.n1;
  fr.d = icp_dot(fr.b1, fr.a2);
  double u[3];
  for (int j = 0; j < 3; ++j) u[j] = fr.a2[j] - fr.d * fr.b1[j];
  const double l2 = sqrt(icp_dot(u, u));
  fr.n2 = l2 < 1e-12 ? 1e-12 : l2;
  for (int j = 0; j < 3; ++j) fr.b2[j] = u[j] / fr.n2;
  double b3[3];
  icp_cross(fr.b1, fr.b2, b3);
  for (int a = 0; a < 3; ++a)
    for (int j = 0; j < 3; ++j)
      xf.R[a * 3 + j] = (float)(((double)ri[a * 3 + 0] * fr.b1[j] + (double)ri[a * 3 + 1] * fr.b2[j]) + (double)ri[a * 3 + 2] * b3[j]);
}

// step 2: THE transformed point; every x of this file comes from here
__device__ __forceinline__ void icp_x(const IcpXf& f, float p0, float p1, float p2, float& x0, float& x1, float& x2) {
#pragma clang fp contract(off)
  const float q0 = f.s[0] * p0, q1 = f.s[1] * p1, q2 = f.s[2] * p2;
  x0 = ((q0 * f.R[0] + q1 * f.R[3]) + q2 * f.R[6]) + f.T[0];
  x1 = ((q0 * f.R[1] + q1 * f.R[4]) + q2 * f.R[7]) + f.T[1];
  x2 = ((q0 * f.R[2] + q1 * f.R[5]) + q2 * f.R[8]) + f.T[2];
}

// steps 3 and 4 for the query of this lane: its 13 terms (all zero for a lane past the last query or without a winner)
template <int DIR>
__device__ __forceinline__ bool icp_pair_terms(const float* __restrict__ pred, int64_t P, const float* __restrict__ gt, int64_t Q,
                                               const IcpXf& f, Vec4<float> (&tile)[NN_TILE], int blk, double (&t)[ICP_TERMS]) {
  const float* __restrict__ qsrc = DIR == 0 ? pred : gt;
  const float* __restrict__ psrc = DIR == 0 ? gt : pred;
  const int64_t NQ = DIR == 0 ? P : Q, NP = DIR == 0 ? Q : P;
  const int64_t q = (int64_t)blk * ICP_THREADS + threadIdx.x;
  const bool live = q < NQ;
  const int64_t qc = live ? q : NQ - 1;                 // clamp: the extra lanes redo the last query and contribute nothing
  const float a0 = qsrc[qc * 3 + 0], a1 = qsrc[qc * 3 + 1], a2 = qsrc[qc * 3 + 2];
  float qx[1] = {a0}, qy[1] = {a1}, qz[1] = {a2};
  if (DIR == 0) icp_x(f, a0, a1, a2, qx[0], qy[0], qz[0]);
  float best[1] = {INFINITY};
  int32_t win[1] = {-1};
  scan_staged<float, 1>(psrc, 0, NP, [&f](float& x, float& y, float& z) { if (DIR == 1) icp_x(f, x, y, z, x, y, z); }, tile, qx, qy, qz, best, win);
  const int32_t bi = win[0];
#pragma unroll
  for (int k = 0; k < ICP_TERMS; ++k) t[k] = 0.0;
  if (!live) return false;
  if (bi < 0) return true;       // no finite distance: no term, and bi is not an index
  float p[3], x[3], y[3];
  if (DIR == 0) {
    p[0] = a0, p[1] = a1, p[2] = a2;
    x[0] = qx[0], x[1] = qy[0], x[2] = qz[0];
    for (int j = 0; j < 3; ++j) y[j] = gt[(int64_t)bi * 3 + j];
  } else {
    y[0] = a0, y[1] = a1, y[2] = a2;
    for (int j = 0; j < 3; ++j) p[j] = pred[(int64_t)bi * 3 + j];
    icp_x(f, p[0], p[1], p[2], x[0], x[1], x[2]);
  }
  const float r0 = x[0] - y[0], r1 = x[1] - y[1], r2 = x[2] - y[2];
  t[0] = (double)((r0 * r0 + r1 * r1) + r2 * r2);
  t[1] = (double)r0, t[2] = (double)r1, t[3] = (double)r2;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    t[4 + 3 * a + 0] = (double)(p[a] * r0);
    t[4 + 3 * a + 1] = (double)(p[a] * r1);
    t[4 + 3 * a + 2] = (double)(p[a] * r2);
  }
  return false;
}

__global__ __launch_bounds__(ICP_THREADS) void icp_pairs_kernel(const float* __restrict__ pred, int64_t P, const float* __restrict__ gt,
                                                                int64_t Q, const float* __restrict__ rot_init,
                                                                const float* __restrict__ params, int nblk0, int nblk1,
                                                                double* __restrict__ part, int32_t* __restrict__ out_flag) {
  __shared__ Vec4<float> tile[NN_TILE];
  __shared__ IcpXf s_xf;
  __shared__ double red[ICP_WAVES][ICP_TERMS];
  const int b = blockIdx.z;
  if (threadIdx.x == 0) {
    IcpXf xf;
    IcpFrame fr;
    icp_rotation(params + (int64_t)b * 12, rot_init + (int64_t)b * 9, xf, fr);
    s_xf = xf;
  }
  __syncthreads();
  const IcpXf f = s_xf;
  double t[ICP_TERMS];
  const bool none = (int)blockIdx.x < nblk0 ? icp_pair_terms<0>(pred, P, gt, Q, f, tile, blockIdx.x, t)
                                            : icp_pair_terms<1>(pred, P, gt, Q, f, tile, blockIdx.x - nblk0, t);
  if (none) atomicOr(out_flag, AM_ICP_NO_NEIGHBOUR);
  // lane -> wave: v[l] += v[l + off]; lanes at and above `off` hold values nobody reads any more
#pragma unroll
  for (int k = 0; k < ICP_TERMS; ++k)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) t[k] += __shfl_down(t[k], off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < ICP_TERMS; ++k) red[wave][k] = t[k];
  __syncthreads();
  // wave -> workgroup, left to right
  if (threadIdx.x < ICP_TERMS) {
    double s = red[0][threadIdx.x];
    for (int w = 1; w < ICP_WAVES; ++w) s += red[w][threadIdx.x];
    part[((int64_t)b * (nblk0 + nblk1) + blockIdx.x) * ICP_TERMS + threadIdx.x] = s;
  }
}

struct IcpUpdate {
  const float* rot_init;
  const double* part;
  double* sums;              // (batch, 2, 13) in the workspace
  int nblk0, nblk1, batch, update;
  double w0, w1, c2, lr, beta1, beta2, eps, bc1, bc2;
  float *params, *adam_m, *adam_v, *best, *out_loss, *out_rot;
  double *out_sums, *out_grad;
};

__global__ __launch_bounds__(ICP_THREADS) void icp_update_kernel(const IcpUpdate u) {
#pragma clang fp contract(off)
  __shared__ float s_loss[ICP_THREADS];
  __shared__ int s_idx[ICP_THREADS];
  const int tid = threadIdx.x;
  // workgroups by index
  const int nblk = u.nblk0 + u.nblk1;
  for (int item = tid; item < u.batch * 2 * ICP_TERMS; item += ICP_THREADS) {
    const int b = item / (2 * ICP_TERMS), dir = item % (2 * ICP_TERMS) / ICP_TERMS, k = item % ICP_TERMS;
    const double* p = u.part + ((int64_t)b * nblk + (dir ? u.nblk0 : 0)) * ICP_TERMS + k;
    const int n = dir ? u.nblk1 : u.nblk0;
    double s = p[0];
    for (int j = 1; j < n; ++j) s += p[(int64_t)j * ICP_TERMS];
    u.sums[item] = s;
    if (u.out_sums) u.out_sums[item] = s;
  }
  __syncthreads();
  float my_loss = INFINITY;
  int my_idx = -1;
  for (int b = tid; b < u.batch; b += ICP_THREADS) {
    const float* prm = u.params + (int64_t)b * 12;
    const float* ri = u.rot_init + (int64_t)b * 9;
    IcpXf xf;
    IcpFrame fr;
    icp_rotation(prm, ri, xf, fr);
    const double* s0 = u.sums + (int64_t)b * 2 * ICP_TERMS;
    double A[ICP_TERMS];
    for (int k = 0; k < ICP_TERMS; ++k) A[k] = u.w0 * s0[k] + u.w1 * s0[ICP_TERMS + k];
    const float loss = (float)A[0];
    double g[12];
    double gR[9];
    for (int a = 0; a < 3; ++a) {
      double M[3];
      for (int j = 0; j < 3; ++j) {
        M[j] = u.c2 * A[4 + 3 * a + j];
        gR[a * 3 + j] = (double)xf.s[a] * M[j];
      }
      g[9 + a] = (M[0] * (double)xf.R[a * 3 + 0] + M[1] * (double)xf.R[a * 3 + 1]) + M[2] * (double)xf.R[a * 3 + 2];
    }
    for (int j = 0; j < 3; ++j) g[j] = u.c2 * A[1 + j];
    double g1[3], g2[3], g3[3], c[3];
    for (int j = 0; j < 3; ++j) {
      g1[j] = ((double)ri[0 + 0] * gR[0 + j] + (double)ri[3 + 0] * gR[3 + j]) + (double)ri[6 + 0] * gR[6 + j];
      g2[j] = ((double)ri[0 + 1] * gR[0 + j] + (double)ri[3 + 1] * gR[3 + j]) + (double)ri[6 + 1] * gR[6 + j];
      g3[j] = ((double)ri[0 + 2] * gR[0 + j] + (double)ri[3 + 2] * gR[3 + j]) + (double)ri[6 + 2] * gR[6 + j];
    }
    icp_cross(fr.b2, g3, c);
    for (int j = 0; j < 3; ++j) g1[j] = g1[j] + c[j];
    icp_cross(g3, fr.b1, c);
    for (int j = 0; j < 3; ++j) g2[j] = g2[j] + c[j];
    const double t2 = icp_dot(g2, fr.b2);
    double gu[3];
    for (int j = 0; j < 3; ++j) gu[j] = (g2[j] - t2 * fr.b2[j]) / fr.n2;
    const double t1 = icp_dot(gu, fr.b1);
    for (int j = 0; j < 3; ++j) g[6 + j] = gu[j] - t1 * fr.b1[j];
    for (int j = 0; j < 3; ++j) g1[j] = g1[j] - (fr.d * gu[j] + t1 * fr.a2[j]);
    const double t0 = icp_dot(g1, fr.b1);
    for (int j = 0; j < 3; ++j) g[3 + j] = (g1[j] - t0 * fr.b1[j]) / fr.n1;
    u.out_loss[b] = loss;
    for (int k = 0; k < 9; ++k) u.out_rot[(int64_t)b * 9 + k] = xf.R[k];
    if (u.out_grad)
      for (int k = 0; k < 12; ++k) u.out_grad[(int64_t)b * 12 + k] = g[k];
    if (u.update) {
      const double step = u.lr / u.bc1, root2 = sqrt(u.bc2);
      for (int k = 0; k < 12; ++k) {
        const int64_t o = (int64_t)b * 12 + k;
        const double m = u.beta1 * (double)u.adam_m[o] + (1.0 - u.beta1) * g[k];
        const double v = u.beta2 * (double)u.adam_v[o] + (1.0 - u.beta2) * (g[k] * g[k]);
        const double denom = sqrt(v) / root2 + u.eps;
        u.adam_m[o] = (float)m;
        u.adam_v[o] = (float)v;
        u.params[o] = (float)((double)prm[k] - step * (m / denom));
      }
    }
    if (loss < my_loss) {        // ascending b inside a lane: the lowest index wins a tie, a NaN never wins
      my_loss = loss;
      my_idx = b;
    }
  }
  if (!u.update) return;
  s_loss[tid] = my_loss;
  s_idx[tid] = my_idx;
  const float old = u.best[15];
  __syncthreads();
  for (int stride = ICP_THREADS / 2; stride >= 1; stride >>= 1) {
    if (tid < stride) {
      const float lo = s_loss[tid + stride];
      const int io = s_idx[tid + stride];
      // a lane without a candidate holds (+inf, -1); among equal losses the lower candidate index
      if (io >= 0 && (s_idx[tid] < 0 || lo < s_loss[tid] || (lo == s_loss[tid] && io < s_idx[tid]))) {
        s_loss[tid] = lo;
        s_idx[tid] = io;
      }
    }
    __syncthreads();
  }
  const int c = s_idx[0];
  const float lc = s_loss[0];
  if (c >= 0 && lc < old && tid < 16) {
    float val = lc;
    if (tid < 9) val = u.out_rot[(int64_t)c * 9 + tid];
    else if (tid < 12) val = u.params[(int64_t)c * 12 + (tid - 9)];
    else if (tid < 15) val = u.params[(int64_t)c * 12 + 9 + (tid - 12)];
    u.best[tid] = val;
  }
}

struct IcpPlan { int nblk0, nblk1; size_t part_bytes, bytes; };
IcpPlan icp_plan(int64_t P, int64_t Q, int batch) {
  IcpPlan pl;
  pl.nblk0 = ceil_div(P, ICP_THREADS);
  pl.nblk1 = ceil_div(Q, ICP_THREADS);
  pl.part_bytes = sizeof(double) * ICP_TERMS * (size_t)batch * ((size_t)pl.nblk0 + pl.nblk1);
  pl.bytes = pl.part_bytes + sizeof(double) * 2 * ICP_TERMS * (size_t)batch;
  return pl;
}

int icp_check(const am_icp_args* a) {
  AM_CHECK(a != nullptr, "am_icp_step: null arguments");
  AM_TRY(check_cloud("am_icp_step", a->batch, a->n_pred, "pred points", 'z'));
  AM_TRY(check_cloud("am_icp_step", a->batch, a->n_gt, "gt points", 'z'));
  AM_CHECK(a->pred && a->gt && a->rot_init && a->params && a->adam_m && a->adam_v && a->best && a->out_loss && a->out_rot && a->out_flag,
           "am_icp_step: null pointer");
  AM_CHECK(!a->update || (a->bias_correction1 > 0.0 && a->bias_correction2 > 0.0),
           "am_icp_step: bias corrections %g / %g must be positive (1 - beta^t of a step count t >= 1)", a->bias_correction1,
           a->bias_correction2);
  return AM_OK;
}

}  // namespace

extern "C" size_t am_icp_workspace_bytes(int64_t n_pred, int64_t n_gt, int batch) {
  return cloud_ok(batch, n_pred) && cloud_ok(batch, n_gt) && batch <= 65535 ? icp_plan(n_pred, n_gt, batch).bytes : 0;
}

extern "C" int am_icp_step(const am_icp_args* a, void* workspace_dev, size_t workspace_bytes, void* stream) {
  AM_TRY(icp_check(a));
  const IcpPlan pl = icp_plan(a->n_pred, a->n_gt, a->batch);
  AM_TRY(check_workspace("am_icp_step", workspace_dev, workspace_bytes, pl.bytes));
  AM_CHECK((uintptr_t)workspace_dev % 8 == 0 && (uintptr_t)a->out_sums % 8 == 0 && (uintptr_t)a->out_grad % 8 == 0,
           "am_icp_step: the workspace, out_sums and out_grad must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  double* part = reinterpret_cast<double*>(workspace_dev);
  hipLaunchKernelGGL(icp_pairs_kernel, dim3(pl.nblk0 + pl.nblk1, 1, a->batch), dim3(ICP_THREADS), 0, st, a->pred, a->n_pred, a->gt, a->n_gt,
                     a->rot_init, a->params, pl.nblk0, pl.nblk1, part, a->out_flag);
  AM_HIP(hipGetLastError());
  IcpUpdate u;
  u.rot_init = a->rot_init;
  u.part = part;
  u.sums = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace_dev) + pl.part_bytes);
  u.nblk0 = pl.nblk0, u.nblk1 = pl.nblk1, u.batch = a->batch, u.update = a->update != 0;
  u.w0 = 1.0 / (double)a->n_pred, u.w1 = 1.0 / (double)a->n_gt, u.c2 = 2.0 / (double)a->batch;
  u.lr = a->lr, u.beta1 = a->beta1, u.beta2 = a->beta2, u.eps = a->eps, u.bc1 = a->bias_correction1, u.bc2 = a->bias_correction2;
  u.params = a->params, u.adam_m = a->adam_m, u.adam_v = a->adam_v, u.best = a->best;
  u.out_loss = a->out_loss, u.out_rot = a->out_rot, u.out_sums = a->out_sums, u.out_grad = a->out_grad;
  hipLaunchKernelGGL(icp_update_kernel, dim3(1), dim3(ICP_THREADS), 0, st, u);
  AM_HIP(hipGetLastError());
  return AM_OK;
}
