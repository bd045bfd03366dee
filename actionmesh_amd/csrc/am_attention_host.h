// Host-side launch plan shared by the attention families (am_attention.hip and am_attention64.hip: bf16 / float16; am_attention_fp8.hip:
// fp8): the argument checks every entry makes, the main / rest boundary of the query blocks, each family's rule for splitting a short
// last block over the key range, and the scratch the split's partials live in.  Host code only.
#pragma once
#include "am_common.h"

constexpr int AM_ATTN_HD = 128;        // head dimension
constexpr int AM_ATTN_KEY_TILE = 64;   // keys per tile: sk_pad is a multiple of it
constexpr int AM_ATTN_SPLIT_Z = 16;    // cuts of a split last block over the key range

// am_attention64.hip: the main (non-split) grid of the 4x64 kernel, query blocks [0, nblk_main) of every (sequence, head)
int am_attention64_main(const am_attn_args* a, int tiles_per_chunk, int nblk_main, int defer, void* stream);
// am_attention.hip: merge of a split last block's partials (256-row query blocks; the fp8 kernel shares the bf16 kernels' partial layout)
int am_attention_combine_launch(const am_attn_args* a, const float* part, int Z, int qblk_base, int rows, void* stream);

// ---- the checks every entry makes (`who`: the entry's name) ---------------------------------------------------------------------------
// What differs on purpose stays in the entry: operands, alignment and ldo, chunk_stride, am_attention_bf16's "chunk_total needs
// rows = 1" and its code list for rows = 1, am_attention_fp8's 32-bit offset check.
static inline int am_attn_check_args(const am_attn_args* a, const char* who) {
  AM_CHECK(a != nullptr, "%s: null args", who);
  AM_CHECK(a->nseq > 0 && a->heads > 0 && a->sq > 0 && a->sk > 0 && a->nchunks > 0, "%s: empty problem", who);
  AM_CHECK(a->sq_pad % 256 == 0 && a->sq_pad >= a->sq, "%s: sq_pad=%d must be a multiple of 256 and >= sq=%d", who, a->sq_pad, a->sq);
  AM_CHECK(a->sk_pad % AM_ATTN_KEY_TILE == 0 && a->sk_pad >= a->sk, "%s: sk_pad=%d must be a multiple of %d and >= sk=%d", who, a->sk_pad,
           AM_ATTN_KEY_TILE, a->sk);
  AM_CHECK(a->rows >= 0 && a->rows <= 2 && a->state_mode >= 0 && a->state_mode <= 2, "%s: bad rows / state_mode", who);
  AM_CHECK(a->state_mode == 0 || (a->rows == 1 && a->state != nullptr && (uintptr_t)a->state % 16 == 0),
           "%s: state_mode needs rows = 1 and a 16-byte aligned state buffer", who);
  AM_CHECK(a->chunk_total == 0 || (a->chunk_total > 0 && a->chunk_first >= 0 && a->chunk_first < a->chunk_total && a->nchunks <= a->chunk_total),
           "%s: chunk_first / chunk_total need 0 <= first < total, nchunks <= total", who);
  AM_CHECK((int64_t)a->nseq * a->heads <= 65535, "%s: nseq*heads=%lld exceeds grid.y", who, (long long)a->nseq * a->heads);
  return AM_OK;
}

// ---- the query-block plan ----------------------------------------------------------------------------------------------------------------
// a->rows: 0 = every query block; 1 = only "main" (all but a short last block); 2 = only what rows = 1 leaves out ("rest").  The boundary
// depends on the query geometry alone - a last block at most half full behind at least eight others - so the calls of a two-pass sequence
// (different nchunks, bf16 or fp8) agree on it.  `qblk_rows`: query rows per workgroup (256; 128 in the 4-wave geometry).
struct am_attn_qblocks {
  int nblk;         // query blocks per (sequence, head)
  int tail_rows;    // valid rows of the last one
  bool tail_rest;   // the last block is "rest"
  int nblk_main;    // blocks that are "main"
};
static inline am_attn_qblocks am_attn_plan_qblocks(const am_attn_args* a, int qblk_rows) {
  am_attn_qblocks q;
  q.nblk = ceil_div(a->sq, qblk_rows);
  q.tail_rows = a->sq - (q.nblk - 1) * qblk_rows;
  q.tail_rest = q.nblk >= 9 && q.tail_rows <= qblk_rows / 2;
  q.nblk_main = q.tail_rest ? q.nblk - 1 : q.nblk;
  return q;
}

// ---- the split of a "rest" block -----------------------------------------------------------------------------------------------------------
// A "rest" block is cut AM_ATTN_SPLIT_Z ways over the key range, and the partials merged by attn_combine_kernel (am_attention.hip), when
// the key stream is long enough for the cuts to pay and the partials fit the cap; otherwise it runs as one ordinary block.  Each family
// has its own measure of "long enough".  (32 cuts instead of 16 change nothing - measured: the pass re-reads every K / V^T byte of the
// launch for 16 query rows, 537 MB at the headline shape = 107 us at 5 TB/s, and sits at 116 us: it is at its HBM floor.)
// Partials: [nseq * heads][AM_ATTN_SPLIT_Z][part_rows][AM_ATTN_STATE_LD] floats, part_rows = the query rows of a splitting workgroup.
static inline size_t am_attn_part_floats(const am_attn_args* a, int part_rows) {
  return (size_t)a->nseq * a->heads * AM_ATTN_SPLIT_Z * part_rows * AM_ATTN_STATE_LD;
}
static inline bool am_attn_part_fits(size_t floats) { return floats * sizeof(float) <= (256u << 20); }
// bf16 / float16: two tiles per cut, and two of the caller's super-tiles (`nsub` tiles each, per chunk)
static inline bool am_attn_bf16_splits(const am_attn_args* a, int nsub, size_t part_floats) {
  const int tiles_per_chunk = ceil_div(a->sk, AM_ATTN_KEY_TILE);
  return (int64_t)tiles_per_chunk * a->nchunks >= 2 * AM_ATTN_SPLIT_Z && ceil_div(tiles_per_chunk, nsub) * a->nchunks >= 2 * AM_ATTN_SPLIT_Z &&
         am_attn_part_fits(part_floats);
}
// fp8: four tiles per cut
static inline bool am_attn_fp8_splits(const am_attn_args* a, size_t part_floats) {
  return ceil_div(a->sk, AM_ATTN_KEY_TILE) * a->nchunks >= 4 * AM_ATTN_SPLIT_Z && am_attn_part_fits(part_floats);
}

// ---- the partials scratch -------------------------------------------------------------------------------------------------------------------
// Library-owned, one buffer per (family, device), grown on demand and never shrunk; growth frees the old buffer and moves
// g_am_scratch_generation (am_common.h).  The families keep separate buffers: their launches may overlap on different streams.  Launches
// on one device are issued from one thread (C-ABI contract).
enum am_attn_family { AM_ATTN_FAMILY_BF16 = 0, AM_ATTN_FAMILY_FP8 = 1 };
int am_attn_partials(am_attn_family family, size_t floats, float** out);   // am_attention.hip: a buffer of at least `floats` floats
