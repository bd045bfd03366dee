// Mesh decimation: the kernels of one round of the parallel quadric edge collapse (actionmesh_amd/mesh_decimate.py), which stands in
// for the reference's trimesh.simplify_quadric_decimation (actionmesh/preprocessing/mesh_processor.py:128-161).  The contract is
// include/actionmesh_amd.h's; all geometry is fp64, every operation rounded on its own (the file is built with -ffp-contract=off), so
// positions, quadrics, costs and keys are compared bit for bit with a numpy restatement.
//
//   am_decimate_quadrics, am_decimate_border_quadrics   one thread per vertex: the area-weighted plane quadrics of its faces, summed in
//                          CSR order (a gather); with `BORDERS` also the two border planes of every corner
//   am_decimate_edges, am_decimate_border_edges   one thread per edge: the topology rule - lock and link tests, with `BORDERS` the three
//                          vertex classes and the coned link condition -, then the Cramer solve or the u / v / midpoint fallback, the
//                          cost, the no-flip test over both stars, the 64-bit key
// `BORDERS` is a template parameter (`borders="collapse"`): one text of each kernel, two instantiations, and the fixed-mode one never reads
// the border tables.
//   am_decimate_select     one thread per vertex, twice (m1: min key of its edges; m2: min of m1 over its closed neighbourhood), then
//                          one thread per edge (selected iff its key is m2 at both ends)
//   am_decimate_apply      one thread per kept edge: moves u, adds the quadrics, rewrites v -> u in v's corners, marks the two faces
// No floating-point atomics anywhere (the only atomic is the OR into the flag word).  No index read from memory is ever used as an
// address before it has been compared with its bound; loops over corners run between CSR offsets that were validated first.
#include "am_geometry.h"

namespace {

constexpr int64_t NO_KEY = AM_DECIMATE_NO_KEY;

__device__ __forceinline__ uint32_t mix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

// the edge index of half-edge h, which runs between vertices a and b; -1 (flag raised) when the table does not say so
__device__ __forceinline__ int edge_of(const mesh_view& m, int h, int a, int b) {
  const int e = m.he2e[h];
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  if (!in_range(e, m.n_edges) || m.edges[2 * (int64_t)e] != lo || m.edges[2 * (int64_t)e + 1] != hi) {
    atomicOr(m.flag, AM_DECIMATE_BAD_EDGE);
    return -1;
  }
  return e;
}

// is w one of the neighbours of v (whose corner range [begin, end) is valid)?
__device__ bool adjacent(const mesh_view& m, int v, int begin, int end, int w) {
  bool found = false;
  for (int j = begin; j < end; ++j) {
    const int c = corner_at(m, j, v);
    if (c < 0) continue;
    const int f3 = c - c % 3, k = c % 3;
    found = found || m.faces[f3 + (k + 1) % 3] == w || m.faces[f3 + (k + 2) % 3] == w;
  }
  return found;
}

// Q[i,j] += (w * P[i]) * P[j] over the upper triangle, P = (n, d)
__device__ __forceinline__ void add_plane(double* q, vec3 n, double d, double w) {
#pragma clang fp contract(off)
  const double p[4] = {n.x, n.y, n.z, d};
  int t = 0;
  for (int a = 0; a < 4; ++a)
    for (int b = a; b < 4; ++b, ++t) q[t] = q[t] + (w * p[a]) * p[b];
}

// ---- what only `BORDERS` reads (the header's "Border collapses") ------------------------------------------------------------------------

// the edge index of half-edge h where only the half-edge table is known; -1 (flag raised) when it is outside [0, n_edges)
__device__ __forceinline__ int edge_index(const mesh_view& m, int h) {
  const int e = m.he2e[h];
  if (!in_range(e, m.n_edges)) {
    atomicOr(m.flag, AM_DECIMATE_BAD_EDGE);
    return -1;
  }
  return e;
}

// the count of edge e (inside [0, n_edges)); a count below 1 raises the flag: every edge of the table has a half-edge
__device__ __forceinline__ int count_of(const mesh_view& m, const int32_t* __restrict__ edge_count, int e) {
  const int n = edge_count[e];
  if (n < 1) atomicOr(m.flag, AM_DECIMATE_BAD_EDGE);
  return n;
}

// one constraint plane of the border half-edge p -> q of a face with unit normal n
__device__ __forceinline__ void add_border_plane(double* q, vec3 p, vec3 pq, vec3 n, double border_weight) {
#pragma clang fp contract(off)
  const vec3 E = sub3(pq, p);
  vec3 mm = cross3(E, n);
  const double ml = norm3(mm);
  if (!(ml > AM_MESH_ZERO)) return;
  mm = div3(mm, ml);
  const double d = -dot3(mm, p);
  add_plane(q, mm, d, border_weight * dot3(E, E));
}

// The gather.  Without BORDERS, edge_count and m.he2e are null and never read, and border_weight is unused.
template <bool BORDERS>
__global__ __launch_bounds__(MESH_THREADS) void decimate_quadrics_kernel(mesh_view m, const double* __restrict__ positions,
                                                                         const int32_t* __restrict__ edge_count, double border_weight,
                                                                         double* __restrict__ out_quadrics) {
#pragma clang fp contract(off)
  const int64_t v = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (v >= m.n_vertices) return;
  double q[10];
  for (int i = 0; i < 10; ++i) q[i] = 0.0;
  int begin, end;
  csr_range(m, (int)v, begin, end);
  for (int j = begin; j < end; ++j) {
    const int c = corner_at(m, j, (int)v);
    if (c < 0) continue;
    const int f3 = c - c % 3, k = c % 3;
    int i[3];
    if (!face_indices(m.faces + f3, m.n_vertices, m.flag, i[0], i[1], i[2])) continue;
    const vec3 p0 = load3(positions, i[0]), p1 = load3(positions, i[1]), p2 = load3(positions, i[2]);
    const vec3 cr = cross3(sub3(p1, p0), sub3(p2, p0));
    const double len = norm3(cr);
    if (!(len > AM_MESH_ZERO)) continue;
    const vec3 n = div3(cr, len);
    add_plane(q, n, -dot3(n, p0), len / 2.0);
    if constexpr (BORDERS) {
      const int hin = f3 + (k + 2) % 3;
      const int eout = edge_index(m, c), ein = edge_index(m, hin);
      const vec3 ps = load3(positions, (int)v);
      if (eout >= 0 && count_of(m, edge_count, eout) == 1) add_border_plane(q, ps, load3(positions, i[(k + 1) % 3]), n, border_weight);
      if (ein >= 0 && count_of(m, edge_count, ein) == 1) add_border_plane(q, load3(positions, i[(k + 2) % 3]), ps, n, border_weight);
    }
  }
  for (int i = 0; i < 10; ++i) out_quadrics[v * 10 + i] = q[i];
}

// y^T Q y with y = (y0, y1, y2, 1)
__device__ __forceinline__ double quadric_cost(const double* q, vec3 y) {
  const double r0 = ((q[0] * y.x + q[1] * y.y) + q[2] * y.z) + q[3];
  const double r1 = ((q[1] * y.x + q[4] * y.y) + q[5] * y.z) + q[6];
  const double r2 = ((q[2] * y.x + q[5] * y.y) + q[7] * y.z) + q[8];
  const double r3 = ((q[3] * y.x + q[6] * y.y) + q[8] * y.z) + q[9];
  return ((r0 * y.x + r1 * y.y) + r2 * y.z) + r3;
}

// One walk over the corners of endpoint s (partner o) for the lock and - on u's side, with v's range - the link counts.
// Returns false when the endpoint is locked or a table is inconsistent.
__device__ bool walk_topology(const mesh_view& m, const int32_t* __restrict__ edge_count, int s, int begin, int end, int o, bool count_link,
                              int obegin, int oend, int* apex, int& n_apex, int& shared) {
  bool ok = true;
  for (int j = begin; j < end; ++j) {
    const int c = corner_at(m, j, s);
    if (c < 0) {
      ok = false;
      continue;
    }
    int w1, w2;
    if (!corner_others(m, c, w1, w2)) {
      ok = false;
      continue;
    }
    const int f3 = c - c % 3, k = c % 3;
    const int e1 = edge_of(m, c, s, w1), e2 = edge_of(m, f3 + (k + 2) % 3, w2, s);
    if (e1 < 0 || e2 < 0 || edge_count[e1] != 2 || edge_count[e2] != 2) ok = false;
    if (!count_link) continue;
    if (w1 == o || w2 == o) {
      if (n_apex < 2) apex[n_apex] = w1 == o ? w2 : w1;
      ++n_apex;
    }
    if (w1 != o && adjacent(m, o, obegin, oend, w1)) ++shared;
    if (w2 != o && adjacent(m, o, obegin, oend, w2)) ++shared;
  }
  return ok;
}

// The no-flip test over the faces of s that do not hold o, with s moved to x; also refuses a face that holds both apexes.
__device__ bool walk_flips(const mesh_view& m, const double* __restrict__ positions, int s, int begin, int end, int o, int a0, int a1,
                           vec3 x) {
#pragma clang fp contract(off)
  bool ok = true;
  for (int j = begin; j < end; ++j) {
    const int c = corner_at(m, j, s);
    if (c < 0) {
      ok = false;
      continue;
    }
    int w1, w2;
    if (!corner_others(m, c, w1, w2)) {
      ok = false;
      continue;
    }
    if (w1 == o || w2 == o) continue;
    if ((w1 == a0 && w2 == a1) || (w1 == a1 && w2 == a0)) ok = false;
    const int k = c % 3;
    vec3 p[3];
    p[k] = load3(positions, s);
    p[(k + 1) % 3] = load3(positions, w1);
    p[(k + 2) % 3] = load3(positions, w2);
    const vec3 c0 = cross3(sub3(p[1], p[0]), sub3(p[2], p[0]));
    p[k] = x;
    const vec3 c1 = cross3(sub3(p[1], p[0]), sub3(p[2], p[0]));
    if (!(dot3(c0, c1) > (AM_DECIMATE_FLIP * sqrt(dot3(c0, c0))) * sqrt(dot3(c1, c1)))) ok = false;
  }
  return ok;
}

// Where a collapse of { u, v } puts the surviving vertex, and what it costs: the Cramer solve on Q_u + Q_v under the conditioning and
// reach rules, else the cheapest of u, v and the midpoint (ties in that order).
__device__ __forceinline__ void place(const double* __restrict__ quadrics, const double* __restrict__ positions, int u, int v, vec3& x,
                                      double& cost) {
#pragma clang fp contract(off)
  double q[10];
  for (int i = 0; i < 10; ++i) q[i] = quadrics[(int64_t)u * 10 + i] + quadrics[(int64_t)v * 10 + i];
  const vec3 pu = load3(positions, u), pv = load3(positions, v);
  const vec3 mid = {(pu.x + pv.x) * 0.5, (pu.y + pv.y) * 0.5, (pu.z + pv.z) * 0.5};
  const vec3 E = sub3(pv, pu);
  const double a = q[0], b = q[1], c = q[2], d = q[4], ee = q[5], f = q[7];
  const double r0 = -q[3], r1 = -q[6], r2 = -q[8];
  const double m0 = d * f - ee * ee, m1 = b * f - ee * c, m2 = b * ee - d * c;
  const double det = (a * m0 - b * m1) + c * m2;
  const double s = r1 * f - ee * r2, t = r1 * ee - d * r2, g = b * r2 - r1 * c;
  const double dx = (r0 * m0 - b * s) + c * t;
  const double dy = (a * s - r0 * m1) + c * g;
  const double dz = (a * (d * r2 - r1 * ee) - b * g) + r0 * m2;
  const double tr = (a + d) + f;
  bool solved = false;
  if (fabs(det) > AM_DECIMATE_COND * ((tr * tr) * tr)) {
    const vec3 y = {dx / det, dy / det, dz / det};
    const vec3 off = sub3(y, mid);
    if (dot3(off, off) <= AM_DECIMATE_REACH * dot3(E, E)) {
      x = y;
      cost = quadric_cost(q, y);
      solved = true;
    }
  }
  if (!solved) {
    x = pu;
    cost = quadric_cost(q, pu);
    const double cv = quadric_cost(q, pv), cm = quadric_cost(q, mid);
    if (cv < cost) {
      x = pv;
      cost = cv;
    }
    if (cm < cost) {
      x = mid;
      cost = cm;
    }
  }
  cost = cost > 0.0 ? cost : 0.0;
}

// The fixed-border rule on an edge { u, v } of count 2: may it collapse, and its two apexes.  Both endpoints are walked whatever the
// first walk found: a bad table entry in either star raises its flag.
__device__ bool fixed_rule(const mesh_view& m, const int32_t* __restrict__ edge_count, int u, int ub, int ue, int v, int vb, int ve,
                           int* apex) {
  int n_apex = 0, shared = 0;
  const bool tu = walk_topology(m, edge_count, u, ub, ue, v, true, vb, ve, apex, n_apex, shared);
  const bool tv = walk_topology(m, edge_count, v, vb, ve, u, false, 0, 0, apex, n_apex, shared);
  if (!(tu && tv && n_apex == 2 && shared == 4)) return false;
  const int a0 = apex[0], a1 = apex[1];           // inside [0, n_vertices): corner_others checked them
  return a0 != a1 && a0 != u && a0 != v && a1 != u && a1 != v && m.offsets[a0 + 1] - m.offsets[a0] > 3 &&
         m.offsets[a1 + 1] - m.offsets[a1] > 3;
}

// What one walk over the corners of an endpoint finds.
struct border_star {
  int n_border = 0;        // count-1 edges at the vertex
  int n_faces = 0;         // faces that hold the partner
  int n_half = 0;          // half-edges between the vertex and the partner
  int apex_border = 0;     // faces that hold the partner whose edge from the vertex to the apex has count 1
  int shared = 0;          // the header's weighted count of neighbours that are the partner's too
  bool plain = true;       // every count is 1 or 2
  bool sound = true;       // no table entry was refused
};

// One walk over the corners of endpoint s (partner o): the class of s and - on u's side, with v's range - the link counts.
__device__ border_star walk_border_topology(const mesh_view& m, const int32_t* __restrict__ edge_count, int s, int begin, int end, int o,
                                            bool count_link, int obegin, int oend, int* apex) {
  border_star t;
  for (int j = begin; j < end; ++j) {
    const int c = corner_at(m, j, s);
    if (c < 0) {
      t.sound = false;
      continue;
    }
    int w1, w2;
    if (!corner_others(m, c, w1, w2)) {
      t.sound = false;
      continue;
    }
    const int f3 = c - c % 3, k = c % 3;
    const int e1 = edge_of(m, c, s, w1), e2 = edge_of(m, f3 + (k + 2) % 3, w2, s);
    if (e1 < 0 || e2 < 0) {
      t.sound = false;
      continue;
    }
    const int c1 = count_of(m, edge_count, e1), c2 = count_of(m, edge_count, e2);
    t.plain = t.plain && (c1 == 1 || c1 == 2) && (c2 == 1 || c2 == 2);
    t.n_border += (c1 == 1) + (c2 == 1);
    t.n_half += (w1 == o) + (w2 == o);
    if (w1 == o || w2 == o) {
      if (count_link && t.n_faces < 2) apex[t.n_faces] = w1 == o ? w2 : w1;
      ++t.n_faces;
      t.apex_border += (w1 == o ? c2 : c1) == 1;
    }
    if (!count_link) continue;
    if (w1 != o && adjacent(m, o, obegin, oend, w1)) t.shared += c1 == 1 ? 2 : 1;
    if (w2 != o && adjacent(m, o, obegin, oend, w2)) t.shared += c2 == 1 ? 2 : 1;
  }
  return t;
}

// Is the coned valence of apex a above 3?  Its face count, plus 2 when it is a border vertex: only an apex of two or three faces is walked.
__device__ bool apex_valence(const mesh_view& m, const int32_t* __restrict__ edge_count, int a) {
  int begin, end;
  if (!csr_range(m, a, begin, end)) return false;
  if (end - begin > 3) return true;
  if (end - begin < 2) return false;
  int apex[2];
  const border_star t = walk_border_topology(m, edge_count, a, begin, end, -1, false, 0, 0, apex);
  return t.sound && t.plain && t.n_border == 2;
}

// The border rule on an edge { u, v } of `count` half-edges: may it collapse, and its apexes (one, apex[0], for a border edge).  v is
// walked only when u passed.
__device__ bool border_rule(const mesh_view& m, const int32_t* __restrict__ edge_count, int count, int u, int ub, int ue, int v, int vb,
                            int ve, int* apex) {
  const border_star su = walk_border_topology(m, edge_count, u, ub, ue, v, true, vb, ve, apex);
  if (su.sound && su.n_half != count) atomicOr(m.flag, AM_DECIMATE_BAD_EDGE);
  bool ok = su.sound && su.n_half == count && (count == 1 || count == 2) && su.plain && (su.n_border == 0 || su.n_border == 2);
  if (!ok) return false;
  const border_star sv = walk_border_topology(m, edge_count, v, vb, ve, u, false, 0, 0, apex);
  ok = sv.sound && sv.plain && (sv.n_border == 0 || sv.n_border == 2) && su.n_faces == count && su.shared == 2 * count;
  ok = ok && ((ue - ub) + su.n_border) + ((ve - vb) + sv.n_border) - 4 > 3;        // the merged vertex's coned valence
  if (count == 2)
    ok = ok && !(su.n_border == 2 && sv.n_border == 2);
  else
    ok = ok && su.apex_border + sv.apex_border < 2;
  if (!ok) return false;
  const int a0 = apex[0], a1 = apex[1];           // a0, and a1 of an interior edge, inside [0, n_vertices): corner_others checked them
  ok = a0 != u && a0 != v && apex_valence(m, edge_count, a0);
  if (count == 2) ok = ok && a0 != a1 && a1 != u && a1 != v && apex_valence(m, edge_count, a1);
  return ok;
}

// The edge evaluation: the rule of the mode between a prologue and a tail that the modes share.  Fixed mode goes on with count-2 edges
// only; with BORDERS the count is read - and a count below 1 flagged - for every edge, a refused one too.
template <bool BORDERS>
__global__ __launch_bounds__(MESH_THREADS) void decimate_edges_kernel(mesh_view m, const double* __restrict__ positions,
                                                                      const double* __restrict__ quadrics,
                                                                      const int32_t* __restrict__ edge_count,
                                                                      double* __restrict__ out_positions, double* __restrict__ out_cost,
                                                                      int64_t* __restrict__ out_key) {
#pragma clang fp contract(off)
  const int64_t e = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (e >= m.n_edges) return;
  const int u = m.edges[2 * e], v = m.edges[2 * e + 1];
  vec3 x = {0.0, 0.0, 0.0};
  double cost = 0.0;
  int64_t key = NO_KEY;
  bool ok = true;
  if (!in_range(u, m.n_vertices) || !in_range(v, m.n_vertices) || u > v) {
    atomicOr(m.flag, AM_DECIMATE_BAD_EDGE);
    ok = false;
  }
  const int count = BORDERS ? count_of(m, edge_count, (int)e) : 2;
  ok = ok && u != v && (BORDERS || edge_count[e] == 2);
  int ub = 0, ue = 0, vb = 0, ve = 0;
  if (ok) {
    const bool ru = csr_range(m, u, ub, ue), rv = csr_range(m, v, vb, ve);
    ok = ru && rv;
  }
  int apex[2] = {-1, -1};
  if (ok) {
    if constexpr (BORDERS)
      ok = border_rule(m, edge_count, count, u, ub, ue, v, vb, ve, apex);
    else
      ok = fixed_rule(m, edge_count, u, ub, ue, v, vb, ve, apex);
  }
  if (ok) {
    place(quadrics, positions, u, v, x, cost);
    const bool fu = walk_flips(m, positions, u, ub, ue, v, apex[0], apex[1], x);       // apex[1] of a border edge is -1: no face holds it
    const bool fv = walk_flips(m, positions, v, vb, ve, u, apex[0], apex[1], x);
    if (fu && fv) key = (int64_t)(((uint64_t)__float_as_uint((float)cost) << 32) | (uint64_t)mix32((uint32_t)e));
  }
  out_positions[3 * e] = x.x;
  out_positions[3 * e + 1] = x.y;
  out_positions[3 * e + 2] = x.z;
  out_cost[e] = cost;
  out_key[e] = key;
}

// pass 0: m1[v] = min key of v's edges;  pass 1: m2[v] = min of m1 over v and its neighbours
__global__ __launch_bounds__(MESH_THREADS) void decimate_min_kernel(mesh_view m, int pass, const int64_t* __restrict__ in,
                                                                    int64_t* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (v >= m.n_vertices) return;
  int64_t best = pass == 0 ? NO_KEY : in[v];
  int begin, end;
  csr_range(m, (int)v, begin, end);
  for (int j = begin; j < end; ++j) {
    const int c = corner_at(m, j, (int)v);
    if (c < 0) continue;
    int w1, w2;
    if (!corner_others(m, c, w1, w2)) continue;
    int64_t k1, k2;
    if (pass == 0) {
      const int f3 = c - c % 3, k = c % 3;
      const int e1 = edge_of(m, c, (int)v, w1), e2 = edge_of(m, f3 + (k + 2) % 3, w2, (int)v);
      k1 = e1 < 0 ? NO_KEY : in[e1];
      k2 = e2 < 0 ? NO_KEY : in[e2];
    } else {
      k1 = in[w1];
      k2 = in[w2];
    }
    best = k1 < best ? k1 : best;
    best = k2 < best ? k2 : best;
  }
  out[v] = best;
}

__global__ __launch_bounds__(MESH_THREADS) void decimate_pick_kernel(mesh_view m, const int64_t* __restrict__ keys,
                                                                     const int64_t* __restrict__ m2, uint8_t* __restrict__ out_selected) {
  const int64_t e = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (e >= m.n_edges) return;
  const int u = m.edges[2 * e], v = m.edges[2 * e + 1];
  uint8_t sel = 0;
  if (!in_range(u, m.n_vertices) || !in_range(v, m.n_vertices) || u > v) {
    atomicOr(m.flag, AM_DECIMATE_BAD_EDGE);
  } else {
    const int64_t k = keys[e];
    sel = (k != NO_KEY && k == m2[u] && k == m2[v]) ? 1 : 0;
  }
  out_selected[e] = sel;
}

__global__ __launch_bounds__(MESH_THREADS) void decimate_apply_kernel(mesh_view m, int64_t n_kept, const int32_t* __restrict__ kept,
                                                                      const double* __restrict__ candidates, double* positions,
                                                                      double* quadrics, int32_t* faces, int32_t* __restrict__ vertex_map,
                                                                      uint8_t* __restrict__ out_face_dead) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
  if (i >= n_kept) return;
  const int e = kept[i];
  if (!in_range(e, m.n_edges)) {
    atomicOr(m.flag, AM_DECIMATE_BAD_KEPT);
    return;
  }
  const int u = m.edges[2 * (int64_t)e], v = m.edges[2 * (int64_t)e + 1];
  if (!in_range(u, m.n_vertices) || !in_range(v, m.n_vertices) || u >= v) {
    atomicOr(m.flag, AM_DECIMATE_BAD_EDGE);
    return;
  }
  int begin, end;
  if (!csr_range(m, v, begin, end)) return;
  for (int c3 = 0; c3 < 3; ++c3) positions[(int64_t)u * 3 + c3] = candidates[(int64_t)e * 3 + c3];
  for (int t = 0; t < 10; ++t) quadrics[(int64_t)u * 10 + t] = quadrics[(int64_t)u * 10 + t] + quadrics[(int64_t)v * 10 + t];
  for (int j = begin; j < end; ++j) {
    const int c = corner_at(m, j, v);       // m.faces is `faces`: this thread alone rewrites the corners of v
    if (c < 0) continue;
    const int f3 = c - c % 3, k = c % 3;
    if (faces[f3 + (k + 1) % 3] == u || faces[f3 + (k + 2) % 3] == u)
      out_face_dead[f3 / 3] = 1;
    else
      faces[c] = u;
  }
  vertex_map[v] = u;
}

int check_edges(const char* who, int64_t n_edges) {
  AM_CHECK(n_edges >= 1 && n_edges <= (((int64_t)1 << 31) - 1), "%s: %lld edges outside 1 .. 2^31 - 1", who, (long long)n_edges);
  return AM_OK;
}

// The gather's launch behind an entry's checks: `a` gives the fields the two argument structs share, the caller those only the border
// struct has (null and 0 in fixed mode).
template <bool BORDERS, class Args>
int launch_quadrics(const Args* a, int64_t n_edges, const int32_t* half_edge_to_edge, const int32_t* edge_count, double border_weight,
                    void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const mesh_view m = {a->n_vertices, a->n_faces, n_edges, a->faces, a->offsets, a->corners, nullptr, half_edge_to_edge, a->out_flag};
  AM_HIP(hipMemsetAsync(a->out_flag, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(decimate_quadrics_kernel<BORDERS>, dim3(mesh_blocks(a->n_vertices)), dim3(MESH_THREADS), 0, st, m, a->positions,
                     edge_count, border_weight, a->out_quadrics);
  AM_HIP(hipGetLastError());
  return AM_OK;
}

// An edge entry whole (the two argument structs have the same fields): the checks in the entry's name `who`, then the launch.
template <bool BORDERS, class Args>
int decimate_edges(const char* who, const Args* a, void* stream) {
  AM_CHECK(a != nullptr, "%s: null arguments", who);
  AM_TRY(check_mesh(who, a->n_vertices, a->n_faces));
  AM_TRY(check_edges(who, a->n_edges));
  AM_CHECK(a->positions && a->quadrics && a->faces && a->offsets && a->corners && a->edges && a->half_edge_to_edge && a->edge_count &&
               a->out_positions && a->out_cost && a->out_key && a->out_flag,
           "%s: null pointer", who);
  hipStream_t st = (hipStream_t)stream;
  const mesh_view m = {a->n_vertices, a->n_faces, a->n_edges, a->faces, a->offsets, a->corners, a->edges, a->half_edge_to_edge, a->out_flag};
  AM_HIP(hipMemsetAsync(a->out_flag, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(decimate_edges_kernel<BORDERS>, dim3(mesh_blocks(a->n_edges)), dim3(MESH_THREADS), 0, st, m, a->positions, a->quadrics,
                     a->edge_count, a->out_positions, a->out_cost, a->out_key);
  AM_HIP(hipGetLastError());
  return AM_OK;
}

}  // namespace

extern "C" int am_decimate_quadrics(const am_decimate_quadrics_args* a, void* stream) {
  AM_CHECK(a != nullptr, "am_decimate_quadrics: null arguments");
  AM_TRY(check_mesh("am_decimate_quadrics", a->n_vertices, a->n_faces));
  AM_CHECK(a->positions && a->faces && a->offsets && a->corners && a->out_quadrics && a->out_flag, "am_decimate_quadrics: null pointer");
  return launch_quadrics<false>(a, 0, nullptr, nullptr, 0.0, stream);
}

extern "C" int am_decimate_edges(const am_decimate_edges_args* a, void* stream) {
  return decimate_edges<false>("am_decimate_edges", a, stream);
}

extern "C" int am_decimate_border_quadrics(const am_decimate_border_quadrics_args* a, void* stream) {
  AM_CHECK(a != nullptr, "am_decimate_border_quadrics: null arguments");
  AM_TRY(check_mesh("am_decimate_border_quadrics", a->n_vertices, a->n_faces));
  AM_TRY(check_edges("am_decimate_border_quadrics", a->n_edges));
  AM_CHECK(a->positions && a->faces && a->offsets && a->corners && a->half_edge_to_edge && a->edge_count && a->out_quadrics && a->out_flag,
           "am_decimate_border_quadrics: null pointer");
  AM_CHECK(a->border_weight >= 0.0 && a->border_weight <= 1.7976931348623157e308,          // a NaN fails the first, an infinity the second
           "am_decimate_border_quadrics: border_weight %g is not finite and >= 0", a->border_weight);
  return launch_quadrics<true>(a, a->n_edges, a->half_edge_to_edge, a->edge_count, a->border_weight, stream);
}

extern "C" int am_decimate_border_edges(const am_decimate_border_edges_args* a, void* stream) {
  return decimate_edges<true>("am_decimate_border_edges", a, stream);
}

extern "C" int am_decimate_select(const am_decimate_select_args* a, void* stream) {
  AM_CHECK(a != nullptr, "am_decimate_select: null arguments");
  AM_TRY(check_mesh("am_decimate_select", a->n_vertices, a->n_faces));
  AM_TRY(check_edges("am_decimate_select", a->n_edges));
  AM_CHECK(a->faces && a->offsets && a->corners && a->edges && a->half_edge_to_edge && a->keys && a->out_m1 && a->out_m2 &&
               a->out_selected && a->out_flag,
           "am_decimate_select: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const mesh_view m = {a->n_vertices, a->n_faces, a->n_edges, a->faces, a->offsets, a->corners, a->edges, a->half_edge_to_edge, a->out_flag};
  AM_HIP(hipMemsetAsync(a->out_flag, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(decimate_min_kernel, dim3(mesh_blocks(a->n_vertices)), dim3(MESH_THREADS), 0, st, m, 0, a->keys, a->out_m1);
  hipLaunchKernelGGL(decimate_min_kernel, dim3(mesh_blocks(a->n_vertices)), dim3(MESH_THREADS), 0, st, m, 1, (const int64_t*)a->out_m1,
                     a->out_m2);
  hipLaunchKernelGGL(decimate_pick_kernel, dim3(mesh_blocks(a->n_edges)), dim3(MESH_THREADS), 0, st, m, a->keys, (const int64_t*)a->out_m2,
                     a->out_selected);
  AM_HIP(hipGetLastError());
  return AM_OK;
}

extern "C" int am_decimate_apply(const am_decimate_apply_args* a, void* stream) {
  AM_CHECK(a != nullptr, "am_decimate_apply: null arguments");
  AM_TRY(check_mesh("am_decimate_apply", a->n_vertices, a->n_faces));
  AM_TRY(check_edges("am_decimate_apply", a->n_edges));
  AM_CHECK(a->n_kept >= 1 && a->n_kept <= a->n_edges, "am_decimate_apply: %lld kept edges outside 1 .. %lld", (long long)a->n_kept,
           (long long)a->n_edges);
  AM_CHECK(a->kept && a->edges && a->candidates && a->offsets && a->corners && a->positions && a->quadrics && a->faces && a->vertex_map &&
               a->out_face_dead && a->out_flag,
           "am_decimate_apply: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const mesh_view m = {a->n_vertices, a->n_faces, a->n_edges, a->faces, a->offsets, a->corners, a->edges, nullptr, a->out_flag};
  AM_HIP(hipMemsetAsync(a->out_flag, 0, sizeof(int32_t), st));
  AM_HIP(hipMemsetAsync(a->out_face_dead, 0, (size_t)a->n_faces, st));
  hipLaunchKernelGGL(decimate_apply_kernel, dim3(mesh_blocks(a->n_kept)), dim3(MESH_THREADS), 0, st, m, a->n_kept, a->kept, a->candidates,
                     a->positions, a->quadrics, a->faces, a->vertex_map, a->out_face_dead);
  AM_HIP(hipGetLastError());
  return AM_OK;
}
