// What the two dense-attention translation units share (dense_attention.hip: exact fp32; dense_attention_split.hip: the bf16
// split arithmetics): which rows a workgroup owns, the statistics of an owned row across its four lane groups, the grid and the
// argument checks of the entry points.
#pragma once

#include "dsphere_mapops.h"

namespace dsph {

constexpr int DA_TILE = 64;  // rows a workgroup owns (16 per wave)

__device__ __forceinline__ float da_group_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16));
  return fmaxf(v, __shfl_xor(v, 32));
}
__device__ __forceinline__ float da_group_sum(float v) {
  v += __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}

// which (map, head, block of 64 rows) a workgroup owns, and the lane's row in it
struct DaBlock {
  int64_t base;   // first row of the map
  int64_t row;    // the lane's owned row
  int64_t ch;     // first channel of the head
  int h;
  bool own;       // row < M
};

__device__ __forceinline__ DaBlock da_block(int64_t M, int heads, int D, int64_t nblk) {
  DaBlock B;
  const int64_t b = blockIdx.x, blk = b % nblk, nh = b / nblk;
  B.h = (int)(nh % heads);
  B.base = (nh / heads) * M;
  B.ch = (int64_t)B.h * D;
  B.row = blk * DA_TILE + (threadIdx.x >> 6) * 16 + (threadIdx.x & 15);
  B.own = B.row < M;
  return B;
}

// workgroups of a launch: one per (map, head, block of 64 rows)
inline int dense_grid(const char* who, int64_t N, int64_t M, int32_t heads, int64_t* nblk, unsigned* grid) {
  *nblk = (M + DA_TILE - 1) / DA_TILE;
  if (N > 0x7fffffffLL / heads || N * heads > 0x7fffffffLL / *nblk) {
    set_error("%s: grid too large (N %lld, heads %d, %lld row blocks)", who, (long long)N, (int)heads, (long long)*nblk);
    return DSPH_E_UNSUPPORTED;
  }
  *grid = (unsigned)(N * heads * *nblk);
  return DSPH_OK;
}

// the shape limits of the kernels, each named in its message
inline int dense_attention_args_ok(const char* who, int64_t ld, int64_t N, int64_t M, int32_t heads, int32_t depth) {
  if (N < 0) { set_error("%s: negative batch size N = %lld", who, (long long)N); return DSPH_E_BADARG; }
  if (M < 1) { set_error("%s: M = %lld rows, must be at least 1", who, (long long)M); return DSPH_E_BADARG; }
  const int rc = attention_shape_ok(who, heads, depth, "");
  return rc != DSPH_OK ? rc : attention_stride_ok(who, ld, heads, depth);
}

}  // namespace dsph
