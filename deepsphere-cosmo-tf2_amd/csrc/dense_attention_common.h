// What the dense-attention sources share (dense_attention_kernel.h: the three flash kernels over an arithmetic policy;
// dense_attention.hip: the exact-fp32 policy and the entry points; dense_attention_split.hip: the bf16 split policy): which rows a
// workgroup owns, the statistics of an owned row across its four lane groups, the mask operand, the statistic a forward leaves for
// its backward, the arguments of a call and their checks.
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

// What the forward leaves per (row, head) for the backward, and how a probability comes back from a logit s.  Unmasked: one float,
// lse = m + log l, p = exp(s scale - lse).  MASKED: the pair buffer (N, M, heads, 2) = (m, log l), read and written as one float2,
// p = exp((x - m) - log l) with x the masked logit: with every key of a row masked m = -1e9 and m + log l rounds back to m, so the
// backward needs the two apart.  (The expressions are the contract: HIP contracts a * b + c, a rewrite can change the last bit.)
template <bool MASKED>
struct DaStat {
  static constexpr int FLOATS = MASKED ? 2 : 1;  // per row, also in the LDS of dk / dv
  float f[FLOATS];
  // of element i = row heads + h (an index, not its parts: dk / dv reads delta[i] beside it, and the two share the arithmetic)
  static __device__ __forceinline__ DaStat load(const float* p, int64_t i) {
    DaStat st;
    if constexpr (MASKED) {
      const float2 t = *reinterpret_cast<const float2*>(p + 2 * i);
      st.f[0] = t.x; st.f[1] = t.y;
    } else {
      st.f[0] = p[i];
    }
    return st;
  }
  // from the running maximum m and sum l of the online softmax
  static __device__ __forceinline__ void store(float* p, int64_t row, int heads, int h, float m, float l) {
    if constexpr (MASKED) {
      *reinterpret_cast<float2*>(p + 2 * (row * heads + h)) = make_float2(m, logf(l));
    } else {
      p[row * heads + h] = m + logf(l);
    }
  }
  // the forward's logit of a key below M
  static __device__ __forceinline__ float logit(float s, float scale, float addend) {
    if constexpr (MASKED) return da_masked_logit(s, scale, addend); else return s * scale;
  }
  __device__ __forceinline__ float prob(float s, float scale, float addend) const {
    if constexpr (MASKED) return __expf((da_masked_logit(s, scale, addend) - f[0]) - f[1]); else return __expf(fmaf(s, scale, -f[0]));
  }
};

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

// A call past its checks, as the launch functions take it.  mk.p == nullptr: no mask, `stat` is lse (N, M, heads); else the pair
// buffer.  The backward fields stay empty in a forward call.
struct DenseCall {
  const float *q, *k, *v;
  int64_t ld;
  float* out;        // (the backward reads it)
  float* stat;
  DaMask mk;
  const float* dout;
  float *delta, *dq, *dk, *dv;
  int64_t ld_grad;
  int64_t N, M;
  int32_t heads, depth, precision;
  int64_t nblk;
  unsigned grid;
  float scale;
  hipStream_t stream;
};

// the split unit's launches (dense_attention_split.hip): precision DSPH_PREC_BF16X6 / _BF16X3, depth 32 or 64, checked by the caller
void dense_split_launch_forward(const DenseCall& c);
void dense_split_launch_backward(const DenseCall& c);

}  // namespace dsph
