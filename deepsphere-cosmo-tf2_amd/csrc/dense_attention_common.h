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

// The mask of the _masked entry points (the reference's `mask` argument): x_ij = s_ij + mask_ij * -1e9, the product rounded to
// fp32, then added in fp32 to the scaled logit -- an ADD, so a fractional mask is a soft bias.  One operand covers every broadcast
// form: element (n, h, i, j) is p[n sb + h sh + i sq + j]; a stride of 0 broadcasts.  Rows need no alignment.  The kernels are
// templates on MASKED with the operand as a trailing parameter pack `MK... mk` -- one DaMask when MASKED, nothing otherwise, so the
// unmasked instantiations keep the kernel arguments, and the code, they had before there was a mask.
struct DaMask {
  const float* p;
  int64_t sb, sh, sq;
};
__device__ __forceinline__ const DaMask& da_mask_of(const DaMask& mk) { return mk; }

constexpr float DA_MASK_WEIGHT = -1e9f;

// the mask row of an owned QUERY row (forward, dq); nullptr for a row past M, whose mask is never read
__device__ __forceinline__ const float* da_mask_row(const DaMask& mk, const DaBlock& B, int64_t M) {
  return B.own ? mk.p + (B.base / M) * mk.sb + B.h * mk.sh + B.row * mk.sq : nullptr;
}

// b[r] = mask[j + r] * -1e9, r = 0..3, the addends of four neighbouring keys of one mask row: one 16-byte load where the address
// allows it, else one load per key below M (a key at or past M is never read; its logit is -inf whatever b holds)
__device__ __forceinline__ void da_mask_addend4(float (&b)[4], const float* row, int64_t j, int64_t M) {
  b[0] = b[1] = b[2] = b[3] = 0.f;
  if (row != nullptr) {
    const float* p = row + j;
    if (j + 3 < M && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
      const float4 t = *reinterpret_cast<const float4*>(p);
      b[0] = t.x; b[1] = t.y; b[2] = t.z; b[3] = t.w;
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (j + r < M) b[r] = p[r];
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) b[r] = __fmul_rn(b[r], DA_MASK_WEIGHT);
}

// the masked logit: (s scale) rounded, + the addend, rounded -- never contracted into one fma
__device__ __forceinline__ float da_masked_logit(float s, float scale, float addend) { return __fadd_rn(__fmul_rn(s, scale), addend); }

// In dk / dv the owned row is the KEY (column B.row of the mask) and the streamed rows are queries.  A key-only mask (sq == 0) is
// one value per lane for the whole kernel; a pair mask is read per query row, 16 lanes on 16 neighbouring floats of one row.
struct DaKeyMask {
  const float* col;  // element (n, h, 0, owned key); nullptr: not owned
  int64_t sq;
  float fixed;       // sq == 0: the addend
};
__device__ __forceinline__ DaKeyMask da_key_mask(const DaMask& mk, const DaBlock& B, int64_t M) {
  DaKeyMask km;
  km.col = B.own ? mk.p + (B.base / M) * mk.sb + B.h * mk.sh + B.row : nullptr;
  km.sq = mk.sq;
  km.fixed = __fmul_rn(km.col != nullptr && mk.sq == 0 ? *km.col : 0.f, DA_MASK_WEIGHT);
  return km;
}
// addends of the queries i .. i + 3 against the owned key (queries at or past M are not read)
__device__ __forceinline__ void da_key_mask_addend4(float (&b)[4], const DaKeyMask& km, int64_t i, int64_t M) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    b[r] = km.fixed;
    if (km.sq != 0 && km.col != nullptr && i + r < M) b[r] = __fmul_rn(km.col[(i + r) * km.sq], DA_MASK_WEIGHT);
  }
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

// the mask operand of a _masked entry point
inline int dense_mask_args_ok(const char* who, const float* mask, int64_t sb, int64_t sh, int64_t sq) {
  if (!mask) { set_error("%s: NULL mask (the unmasked entry points take none)", who); return DSPH_E_BADARG; }
  if (sb < 0 || sh < 0 || sq < 0) {
    set_error("%s: negative mask stride (batch %lld, head %lld, query %lld); 0 broadcasts", who, (long long)sb, (long long)sh, (long long)sq);
    return DSPH_E_BADARG;
  }
  return DSPH_OK;
}

// The fp32 kernels of the _masked entry points (dense_attention.hip); arguments checked by the caller (dense_attention_split.hip,
// where the entry points live beside the precision dispatch).  `stat` is the pair buffer (N, M, heads, 2) = (m, log l).
int dense_attention_forward_masked_fp32(const float* q, const float* k, const float* v, int64_t ld, float* out, float* stat, const DaMask& mk,
                                        int64_t N, int64_t M, int32_t heads, int32_t depth, hipStream_t stream);
int dense_attention_backward_masked_fp32(const float* q, const float* k, const float* v, int64_t ld, const float* out, const float* stat,
                                         const DaMask& mk, const float* dout, float* delta, float* dq, float* dk, float* dv, int64_t ld_grad,
                                         int64_t N, int64_t M, int32_t heads, int32_t depth, hipStream_t stream);

}  // namespace dsph
