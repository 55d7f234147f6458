// Dense attention: every row attends to every row of its map (the super-pixel tokens of Graph_ViT).  Replaces
// gnn_transformers.scaled_dot_product_attention of the reference (gnn_transformers.py:14-51), which materialises the logits and the
// attention weights as two (N, heads, M, M) tensors; here no logit ever reaches global memory (flash attention: online softmax
// over key tiles, the backward recomputes the probabilities from the log-sum-exp).
//
//   s_ij = q_i,h . k_j,h / sqrt(D)     p_ij = softmax_j(s_ij), j over ALL rows     out_i,h = sum_j p_ij v_j,h     lse_i,h = log sum_j exp(s_ij)
//
// Layout: as nbr_attention.hip -- q, k, v channels-last (N, M, d) with a row stride ld >= d (three views of one (N, M, 3 d)
// projection), heads are contiguous groups of D channels; out (N, M, d) and lse (N, M, heads) contiguous.
//
// A workgroup (4 waves) owns DA_TILE = 64 rows of one (map, head), a wave 16 of them, and streams the other side through LDS in
// tiles of 64 rows; the next tile's global loads are in flight while the current one is computed.  All products run on the
// exact-fp32 MFMA v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain, no reduced precision, no range condition).  The products are
// taken TRANSPOSED: S^T = T O^T with the streamed rows T (from LDS) as the A operand and the owned rows O (a register fragment,
// loaded once) as B, so a lane holds s[r] = S(tile row 4 (lane / 16) + r, owned row lane % 16).  That is, register by register,
// the B operand of the second product acc^T += T'^T X^T (X = P or dS; T' = the V, K, Q or dout tile) when step r of it sums
// over the tile rows 4 g + r, g = 0..3 -- the A operand is read from LDS under that permutation -- so the softmax feeds the
// second MFMA without passing through LDS.  The statistics of an owned row live in its lane: a maximum / sum over a tile is one
// over 16 registers and the 4 lane groups (two xor shuffles).
//
// LDS tiles are [64][D + 4] floats (D = 4: [64][4]): rows 16 bytes aligned, and both read patterns (16 rows x 4 channel groups
// for the first product, 4 rows x 16 channels for the second) fall on 64 different banks.  Tails: rows past M of a streamed tile
// are zero-filled and their logits masked (p = 0); owned rows past M compute on zeros and store nothing.
//
// Backward, no atomics, bitwise reproducible.  With delta_i,h = dout_i,h . out_i,h and p_ij = exp(s_ij - lse_i):
//   pass 1, query blocks, over key tiles:    ds_ij = p_ij (dout_i . v_j - delta_i)    dq_i = scale sum_j ds_ij k_j     (writes delta)
//   pass 2, key blocks, over query tiles:    dv_j = sum_i p_ij dout_i                 dk_j = scale sum_i ds_ij q_i
// Two launches on the caller's stream; every output element has one writer and a fixed order of summation.
#include <cmath>

#include "dense_attention_common.h"

namespace dsph {

typedef float da_f32x4 __attribute__((ext_vector_type(4)));

template <int D>
struct DaShape {
  static constexpr int STRIDE = D == 4 ? 4 : D + 4;               // floats between the rows of an LDS tile
  static constexpr int NF = D / 4;                                // registers of a lane's row fragment = MFMA steps of a dot product
  static constexpr int CB = (D + 15) / 16;                        // 16-channel blocks of the accumulator
  static constexpr int STAGE = (DA_TILE * (D / 4) + 255) / 256;   // 16-byte pieces of a tile per thread
};

// A lane's fragment of one row: the channels that its lane group g = lane / 16 contributes to the dot product, fragment element e
// being MFMA step e (both operands use this one map, so any map is right; this one makes the loads 16 bytes wide).
// D >= 16: element 4 b + s is channel 16 b + 4 g + s;  D = 8: element s is channel 2 g + s;  D = 4: channel g.
template <int D>
__device__ __forceinline__ void da_load_frag(float (&f)[DaShape<D>::NF], const float* row, int g) {
  if constexpr (D >= 16) {
#pragma unroll
    for (int b = 0; b < D / 16; ++b) {
      const float4 t = *reinterpret_cast<const float4*>(row + 16 * b + 4 * g);
      f[4 * b] = t.x; f[4 * b + 1] = t.y; f[4 * b + 2] = t.z; f[4 * b + 3] = t.w;
    }
  } else if constexpr (D == 8) {
    const float2 t = *reinterpret_cast<const float2*>(row + 2 * g);
    f[0] = t.x; f[1] = t.y;
  } else {
    f[0] = row[g];
  }
}

template <int D>
__device__ __forceinline__ void da_zero_frag(float (&f)[DaShape<D>::NF]) {
#pragma unroll
  for (int e = 0; e < DaShape<D>::NF; ++e) f[e] = 0.f;
}

// c[r] = (row 16 sub + 4 g + r of the LDS tile) . (the owned row of lane % 16, fragment `own`)
template <int D>
__device__ __forceinline__ da_f32x4 da_tile_dot(const float* tile, int sub, const float (&own)[DaShape<D>::NF], int lane) {
  float a[DaShape<D>::NF];
  da_load_frag<D>(a, tile + (16 * sub + (lane & 15)) * DaShape<D>::STRIDE, lane >> 4);
  da_f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < DaShape<D>::NF; ++e) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], own[e], c, 0, 0, 0);
  return c;
}

// acc[b][r'] (channel 16 b + 4 g + r', owned row lane % 16) += sum over the tile rows t = 16 sub + 4 g' + r of tile[t][channel] x(t),
// x(t) being register r of the lanes of group g': what da_tile_dot returned, after the softmax
template <int D>
__device__ __forceinline__ void da_tile_acc(da_f32x4 (&acc)[DaShape<D>::CB], const float* tile, int sub, const da_f32x4& x, int lane) {
  const int g = lane >> 4, c = lane & 15;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float* row = tile + (16 * sub + 4 * g + r) * DaShape<D>::STRIDE;
#pragma unroll
    for (int b = 0; b < DaShape<D>::CB; ++b) {
      float a;
      if constexpr (D >= 16) {
        a = row[16 * b + c];
      } else {  // (lanes past the head's channels: a zero row of the A operand)
        a = row[c < D ? c : 0];
        a = c < D ? a : 0.f;
      }
      acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, x[r], acc[b], 0, 0, 0);
    }
  }
}

// a tile of `valid` (<= 64) rows, D channels from src on, rows ld apart: global -> registers, registers -> LDS (zeros past `valid`)
template <int D>
__device__ __forceinline__ void da_stage_load(float4 (&s)[DaShape<D>::STAGE], const float* __restrict__ src, int64_t ld, int valid, int tid) {
#pragma unroll
  for (int i = 0; i < DaShape<D>::STAGE; ++i) {
    const int idx = tid + 256 * i, row = idx / (D / 4), c4 = idx % (D / 4);
    s[i] = row < valid ? *reinterpret_cast<const float4*>(src + row * ld + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

template <int D>
__device__ __forceinline__ void da_stage_store(const float4 (&s)[DaShape<D>::STAGE], float* tile, int tid) {
#pragma unroll
  for (int i = 0; i < DaShape<D>::STAGE; ++i) {
    const int idx = tid + 256 * i, row = idx / (D / 4), c4 = idx % (D / 4);
    if (row < DA_TILE) *reinterpret_cast<float4*>(tile + row * DaShape<D>::STRIDE + 4 * c4) = s[i];
  }
}

// the lane's accumulator, times f, to channels [16 b + 4 g, + 4) of its row
template <int D>
__device__ __forceinline__ void da_store_acc(float* rowp, const da_f32x4 (&acc)[DaShape<D>::CB], float f, int g) {
#pragma unroll
  for (int b = 0; b < DaShape<D>::CB; ++b)
    if (16 * b + 4 * g < D) *reinterpret_cast<float4*>(rowp + 16 * b + 4 * g) = make_float4(acc[b][0] * f, acc[b][1] * f, acc[b][2] * f, acc[b][3] * f);
}

// MASKED: the logits take the mask's addend (dense_attention_common.h) and `lse` is the pair buffer (N, M, heads, 2) = (m, log l):
// with every key of a row masked m = -1e9 and m + log l rounds back to m, so the backward needs the two apart.
template <int D, bool MASKED = false, typename... MK>
__global__ __launch_bounds__(256) void dense_attention_forward_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                       const float* __restrict__ v, int64_t ld, float* __restrict__ out,
                                                                       float* __restrict__ lse, int64_t M, int heads, int64_t nblk,
                                                                       float scale, MK... mk) {
  using S = DaShape<D>;
  __shared__ __attribute__((aligned(16))) float sk[DA_TILE * S::STRIDE];
  __shared__ __attribute__((aligned(16))) float sv[DA_TILE * S::STRIDE];
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
  const DaBlock B = da_block(M, heads, D, nblk);
  float qf[S::NF];
  if (B.own) da_load_frag<D>(qf, q + (B.base + B.row) * ld + B.ch, g); else da_zero_frag<D>(qf);
  da_f32x4 acc[S::CB];
#pragma unroll
  for (int b = 0; b < S::CB; ++b) acc[b] = da_f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -__builtin_huge_valf(), l = 0.f;
  const float* mrow = nullptr;
  if constexpr (MASKED) mrow = da_mask_row(da_mask_of(mk...), B, M);
  const int64_t ntiles = (M + DA_TILE - 1) / DA_TILE;
  float4 pk[S::STAGE], pv[S::STAGE];
  {
    const int valid = (int)(M < DA_TILE ? M : DA_TILE);
    da_stage_load<D>(pk, k + B.base * ld + B.ch, ld, valid, tid);
    da_stage_load<D>(pv, v + B.base * ld + B.ch, ld, valid, tid);
    da_stage_store<D>(pk, sk, tid);
    da_stage_store<D>(pv, sv, tid);
  }
  __syncthreads();
  for (int64_t t = 0; t < ntiles; ++t) {
    const int64_t j0 = t * DA_TILE;
    if (t + 1 < ntiles) {
      const int64_t left = M - (j0 + DA_TILE);
      const int valid = (int)(left < DA_TILE ? left : DA_TILE);
      da_stage_load<D>(pk, k + (B.base + j0 + DA_TILE) * ld + B.ch, ld, valid, tid);
      da_stage_load<D>(pv, v + (B.base + j0 + DA_TILE) * ld + B.ch, ld, valid, tid);
    }
    da_f32x4 s[4];
    float mx = -__builtin_huge_valf();
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      float mb[4];
      if constexpr (MASKED) da_mask_addend4(mb, mrow, j0 + 16 * sub + 4 * g, M);
      s[sub] = da_tile_dot<D>(sk, sub, qf, lane);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if constexpr (MASKED) {
          s[sub][r] = j0 + 16 * sub + 4 * g + r < M ? da_masked_logit(s[sub][r], scale, mb[r]) : -__builtin_huge_valf();
        } else {
          s[sub][r] = j0 + 16 * sub + 4 * g + r < M ? s[sub][r] * scale : -__builtin_huge_valf();
        }
        mx = fmaxf(mx, s[sub][r]);
      }
    }
    const float mn = fmaxf(m, da_group_max(mx));  // (finite: a tile holds at least one row below M)
    const float corr = __expf(m - mn);            // (first tile: m = -inf, corr = 0)
    float sum = 0.f;
#pragma unroll
    for (int sub = 0; sub < 4; ++sub)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[sub][r] = __expf(s[sub][r] - mn);
        sum += s[sub][r];
      }
    l = fmaf(l, corr, da_group_sum(sum));
    m = mn;
#pragma unroll
    for (int b = 0; b < S::CB; ++b) acc[b] *= corr;
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) da_tile_acc<D>(acc, sv, sub, s[sub], lane);
    __syncthreads();
    if (t + 1 < ntiles) {
      da_stage_store<D>(pk, sk, tid);
      da_stage_store<D>(pv, sv, tid);
    }
    __syncthreads();
  }
  if (!B.own) return;
  da_store_acc<D>(out + (B.base + B.row) * ((int64_t)heads * D) + B.ch, acc, 1.f / l, g);
  if (lse != nullptr && g == 0) {
    if constexpr (MASKED) {
      *reinterpret_cast<float2*>(lse + 2 * ((B.base + B.row) * heads + B.h)) = make_float2(m, logf(l));
    } else {
      lse[(B.base + B.row) * heads + B.h] = m + logf(l);
    }
  }
}

// pass 1 of the backward: delta and dq of the owned query rows, over the key tiles
template <int D, bool MASKED = false, typename... MK>
__global__ __launch_bounds__(256) void dense_attention_dq_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                  const float* __restrict__ v, int64_t ld, const float* __restrict__ out,
                                                                  const float* __restrict__ lse, const float* __restrict__ dout,
                                                                  float* __restrict__ delta, float* __restrict__ dq, int64_t ldg, int64_t M,
                                                                  int heads, int64_t nblk, float scale,
                                                                  MK... mk) {
  using S = DaShape<D>;
  __shared__ __attribute__((aligned(16))) float sk[DA_TILE * S::STRIDE];
  __shared__ __attribute__((aligned(16))) float sv[DA_TILE * S::STRIDE];
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
  const DaBlock B = da_block(M, heads, D, nblk);
  const int64_t d = (int64_t)heads * D;
  float qf[S::NF], gf[S::NF];
  float dl = 0.f, ls = 0.f;
  float ll = 0.f;            // MASKED: (ls, ll) = (m, log l) of the owned row
  const float* mrow = nullptr;
  if constexpr (MASKED) mrow = da_mask_row(da_mask_of(mk...), B, M);
  if (B.own) {
    float of[S::NF];
    da_load_frag<D>(qf, q + (B.base + B.row) * ld + B.ch, g);
    da_load_frag<D>(gf, dout + (B.base + B.row) * d + B.ch, g);
    da_load_frag<D>(of, out + (B.base + B.row) * d + B.ch, g);
#pragma unroll
    for (int e = 0; e < S::NF; ++e) dl = fmaf(gf[e], of[e], dl);
    if constexpr (MASKED) {
      const float2 st = *reinterpret_cast<const float2*>(lse + 2 * ((B.base + B.row) * heads + B.h));
      ls = st.x; ll = st.y;
    } else {
      ls = lse[(B.base + B.row) * heads + B.h];
    }
  } else {
    da_zero_frag<D>(qf);
    da_zero_frag<D>(gf);
  }
  dl = da_group_sum(dl);  // (the four lane groups of a row hold its D channels once)
  da_f32x4 acc[S::CB];
#pragma unroll
  for (int b = 0; b < S::CB; ++b) acc[b] = da_f32x4{0.f, 0.f, 0.f, 0.f};
  const int64_t ntiles = (M + DA_TILE - 1) / DA_TILE;
  float4 pk[S::STAGE], pv[S::STAGE];
  {
    const int valid = (int)(M < DA_TILE ? M : DA_TILE);
    da_stage_load<D>(pk, k + B.base * ld + B.ch, ld, valid, tid);
    da_stage_load<D>(pv, v + B.base * ld + B.ch, ld, valid, tid);
    da_stage_store<D>(pk, sk, tid);
    da_stage_store<D>(pv, sv, tid);
  }
  __syncthreads();
  for (int64_t t = 0; t < ntiles; ++t) {
    const int64_t j0 = t * DA_TILE;
    if (t + 1 < ntiles) {
      const int64_t left = M - (j0 + DA_TILE);
      const int valid = (int)(left < DA_TILE ? left : DA_TILE);
      da_stage_load<D>(pk, k + (B.base + j0 + DA_TILE) * ld + B.ch, ld, valid, tid);
      da_stage_load<D>(pv, v + (B.base + j0 + DA_TILE) * ld + B.ch, ld, valid, tid);
    }
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      float mb[4];
      if constexpr (MASKED) da_mask_addend4(mb, mrow, j0 + 16 * sub + 4 * g, M);
      const da_f32x4 s = da_tile_dot<D>(sk, sub, qf, lane);
      const da_f32x4 dp = da_tile_dot<D>(sv, sub, gf, lane);
      da_f32x4 ds;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float p;
        if constexpr (MASKED) {
          p = j0 + 16 * sub + 4 * g + r < M ? __expf((da_masked_logit(s[r], scale, mb[r]) - ls) - ll) : 0.f;
        } else {
          p = j0 + 16 * sub + 4 * g + r < M ? __expf(fmaf(s[r], scale, -ls)) : 0.f;
        }
        ds[r] = p * (dp[r] - dl);
      }
      da_tile_acc<D>(acc, sk, sub, ds, lane);
    }
    __syncthreads();
    if (t + 1 < ntiles) {
      da_stage_store<D>(pk, sk, tid);
      da_stage_store<D>(pv, sv, tid);
    }
    __syncthreads();
  }
  if (!B.own) return;
  if (g == 0) delta[(B.base + B.row) * heads + B.h] = dl;
  da_store_acc<D>(dq + (B.base + B.row) * ldg + B.ch, acc, scale, g);
}

// pass 2: dk and dv of the owned key rows, over the query tiles (q and dout rows in LDS, their lse and delta beside them)
template <int D, bool MASKED = false, typename... MK>
__global__ __launch_bounds__(256) void dense_attention_dkv_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                   const float* __restrict__ v, int64_t ld, const float* __restrict__ lse,
                                                                   const float* __restrict__ dout, const float* __restrict__ delta,
                                                                   float* __restrict__ dk, float* __restrict__ dv, int64_t ldg, int64_t M,
                                                                   int heads, int64_t nblk, float scale,
                                                                   MK... mk) {
  using S = DaShape<D>;
  constexpr int ST = MASKED ? 2 : 1;  // floats of a row's statistic: lse, or m and, DA_TILE further on, log l
  __shared__ __attribute__((aligned(16))) float sq[DA_TILE * S::STRIDE];
  __shared__ __attribute__((aligned(16))) float sg[DA_TILE * S::STRIDE];
  __shared__ __attribute__((aligned(16))) float sl[ST * DA_TILE];
  __shared__ __attribute__((aligned(16))) float sd[DA_TILE];
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
  const DaBlock B = da_block(M, heads, D, nblk);
  const int64_t d = (int64_t)heads * D;
  float kf[S::NF], vf[S::NF];
  if (B.own) {
    da_load_frag<D>(kf, k + (B.base + B.row) * ld + B.ch, g);
    da_load_frag<D>(vf, v + (B.base + B.row) * ld + B.ch, g);
  } else {
    da_zero_frag<D>(kf);
    da_zero_frag<D>(vf);
  }
  da_f32x4 ak[S::CB], av[S::CB];
#pragma unroll
  for (int b = 0; b < S::CB; ++b) ak[b] = av[b] = da_f32x4{0.f, 0.f, 0.f, 0.f};
  const int64_t ntiles = (M + DA_TILE - 1) / DA_TILE;
  float4 pq[S::STAGE], pg[S::STAGE];
  float pl = 0.f, pd = 0.f;  // threads 0..63: lse and delta of tile row tid
  float pl2 = 0.f;           // MASKED: (pl, pl2) = (m, log l)
  DaKeyMask km;
  if constexpr (MASKED) km = da_key_mask(da_mask_of(mk...), B, M);
  {
    const int valid = (int)(M < DA_TILE ? M : DA_TILE);
    da_stage_load<D>(pq, q + B.base * ld + B.ch, ld, valid, tid);
    da_stage_load<D>(pg, dout + B.base * d + B.ch, d, valid, tid);
    if (tid < valid) {
      if constexpr (MASKED) {
        const float2 st = *reinterpret_cast<const float2*>(lse + 2 * ((B.base + tid) * heads + B.h));
        pl = st.x; pl2 = st.y;
      } else {
        pl = lse[(B.base + tid) * heads + B.h];
      }
      pd = delta[(B.base + tid) * heads + B.h];
    }
    da_stage_store<D>(pq, sq, tid);
    da_stage_store<D>(pg, sg, tid);
    if (tid < DA_TILE) {
      sl[tid] = pl; sd[tid] = pd;
      if constexpr (MASKED) sl[DA_TILE + tid] = pl2;
    }
  }
  __syncthreads();
  for (int64_t t = 0; t < ntiles; ++t) {
    const int64_t i0 = t * DA_TILE;
    if (t + 1 < ntiles) {
      const int64_t left = M - (i0 + DA_TILE);
      const int valid = (int)(left < DA_TILE ? left : DA_TILE);
      da_stage_load<D>(pq, q + (B.base + i0 + DA_TILE) * ld + B.ch, ld, valid, tid);
      da_stage_load<D>(pg, dout + (B.base + i0 + DA_TILE) * d + B.ch, d, valid, tid);
      pl = pd = pl2 = 0.f;
      if (tid < valid) {
        if constexpr (MASKED) {
          const float2 st = *reinterpret_cast<const float2*>(lse + 2 * ((B.base + i0 + DA_TILE + tid) * heads + B.h));
          pl = st.x; pl2 = st.y;
        } else {
          pl = lse[(B.base + i0 + DA_TILE + tid) * heads + B.h];
        }
        pd = delta[(B.base + i0 + DA_TILE + tid) * heads + B.h];
      }
    }
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
      const da_f32x4 s = da_tile_dot<D>(sq, sub, kf, lane);   // s[r]: query i0 + 16 sub + 4 g + r, the lane's key
      const da_f32x4 dp = da_tile_dot<D>(sg, sub, vf, lane);
      const float4 l4 = *reinterpret_cast<const float4*>(sl + 16 * sub + 4 * g);
      const float4 d4 = *reinterpret_cast<const float4*>(sd + 16 * sub + 4 * g);
      const float lq[4] = {l4.x, l4.y, l4.z, l4.w}, dq4[4] = {d4.x, d4.y, d4.z, d4.w};
      float mb[4], lq2[4];
      if constexpr (MASKED) {
        da_key_mask_addend4(mb, km, i0 + 16 * sub + 4 * g, M);
        const float4 t = *reinterpret_cast<const float4*>(sl + DA_TILE + 16 * sub + 4 * g);
        lq2[0] = t.x; lq2[1] = t.y; lq2[2] = t.z; lq2[3] = t.w;
      }
      da_f32x4 p, ds;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if constexpr (MASKED) {
          p[r] = i0 + 16 * sub + 4 * g + r < M ? __expf((da_masked_logit(s[r], scale, mb[r]) - lq[r]) - lq2[r]) : 0.f;
        } else {
          p[r] = i0 + 16 * sub + 4 * g + r < M ? __expf(fmaf(s[r], scale, -lq[r])) : 0.f;
        }
        ds[r] = p[r] * (dp[r] - dq4[r]);
      }
      da_tile_acc<D>(av, sg, sub, p, lane);
      da_tile_acc<D>(ak, sq, sub, ds, lane);
    }
    __syncthreads();
    if (t + 1 < ntiles) {
      da_stage_store<D>(pq, sq, tid);
      da_stage_store<D>(pg, sg, tid);
      if (tid < DA_TILE) {
        sl[tid] = pl; sd[tid] = pd;
        if constexpr (MASKED) sl[DA_TILE + tid] = pl2;
      }
    }
    __syncthreads();
  }
  if (!B.own) return;
  da_store_acc<D>(dv + (B.base + B.row) * ldg + B.ch, av, 1.f, g);
  da_store_acc<D>(dk + (B.base + B.row) * ldg + B.ch, ak, scale, g);
}

#define DENSE_BY_DEPTH(depth, CALL) \
  switch (depth) {                  \
    case 4: CALL(4); break;         \
    case 8: CALL(8); break;         \
    case 16: CALL(16); break;       \
    case 32: CALL(32); break;       \
    default: CALL(64); break;       \
  }

// the masked launches (arguments checked by the entry points in dense_attention_split.hip)
int dense_attention_forward_masked_fp32(const float* q, const float* k, const float* v, int64_t ld, float* out, float* stat, const DaMask& mk,
                                        int64_t N, int64_t M, int32_t heads, int32_t depth, hipStream_t stream) {
  int64_t nblk;
  unsigned grid;
  const int rc = dense_grid("dense_attention_forward_masked", N, M, heads, &nblk, &grid);
  if (rc != DSPH_OK) return rc;
  const float scale = (float)(1.0 / std::sqrt((double)depth));
#define DENSE_FWD(DD)                                                                                                                  \
  hipLaunchKernelGGL((dense_attention_forward_kernel<DD, true, DaMask>), dim3(grid), dim3(256), 0, stream, q, k, v, ld, out, stat, M, (int)heads, \
                     nblk, scale, mk)
  DENSE_BY_DEPTH(depth, DENSE_FWD)
#undef DENSE_FWD
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

int dense_attention_backward_masked_fp32(const float* q, const float* k, const float* v, int64_t ld, const float* out, const float* stat,
                                         const DaMask& mk, const float* dout, float* delta, float* dq, float* dk, float* dv, int64_t ld_grad,
                                         int64_t N, int64_t M, int32_t heads, int32_t depth, hipStream_t stream) {
  int64_t nblk;
  unsigned grid;
  const int rc = dense_grid("dense_attention_backward_masked", N, M, heads, &nblk, &grid);
  if (rc != DSPH_OK) return rc;
  const float scale = (float)(1.0 / std::sqrt((double)depth));
#define DENSE_BWD(DD)                                                                                                                     \
  hipLaunchKernelGGL((dense_attention_dq_kernel<DD, true, DaMask>), dim3(grid), dim3(256), 0, stream, q, k, v, ld, out, stat, dout, delta, dq,    \
                     ld_grad, M, (int)heads, nblk, scale, mk);                                                                            \
  hipLaunchKernelGGL((dense_attention_dkv_kernel<DD, true, DaMask>), dim3(grid), dim3(256), 0, stream, q, k, v, ld, stat, dout, delta, dk, dv,    \
                     ld_grad, M, (int)heads, nblk, scale, mk)
  DENSE_BY_DEPTH(depth, DENSE_BWD)
#undef DENSE_BWD
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

}  // namespace dsph

extern "C" {

int dsph_dense_attention_forward(const float* q, const float* k, const float* v, int64_t ld, float* out, float* lse, int64_t N, int64_t M,
                                 int32_t heads, int32_t depth, int device, void* hip_stream) {
  using namespace dsph;
  if (!q || !k || !v || !out) { set_error("dense_attention_forward: NULL pointer"); return DSPH_E_BADARG; }
  int rc = dense_attention_args_ok("dense_attention_forward", ld, N, M, heads, depth);
  if (rc != DSPH_OK) return rc;
  if (!aligned16({q, k, v, out})) { set_error("dense_attention_forward: q, k, v and out must be 16-byte aligned"); return DSPH_E_BADARG; }
  DeviceGuard guard(device);
  if (N <= 0 || M <= 0) return DSPH_OK;
  int64_t nblk;
  unsigned grid;
  rc = dense_grid("dense_attention_forward", N, M, heads, &nblk, &grid);
  if (rc != DSPH_OK) return rc;
  const float scale = (float)(1.0 / std::sqrt((double)depth));
  hipStream_t stream = (hipStream_t)hip_stream;
#define DENSE_FWD(DD) \
  hipLaunchKernelGGL(dense_attention_forward_kernel<DD>, dim3(grid), dim3(256), 0, stream, q, k, v, ld, out, lse, M, (int)heads, nblk, scale)
  DENSE_BY_DEPTH(depth, DENSE_FWD)
#undef DENSE_FWD
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

int dsph_dense_attention_backward(const float* q, const float* k, const float* v, int64_t ld, const float* out, const float* lse,
                                  const float* dout, float* delta, float* dq, float* dk, float* dv, int64_t ld_grad, int64_t N, int64_t M,
                                  int32_t heads, int32_t depth, int device, void* hip_stream) {
  using namespace dsph;
  if (!q || !k || !v || !out || !lse || !dout || !delta || !dq || !dk || !dv) {
    set_error("dense_attention_backward: NULL pointer");
    return DSPH_E_BADARG;
  }
  int rc = dense_attention_args_ok("dense_attention_backward", ld, N, M, heads, depth);
  if (rc == DSPH_OK) rc = dense_attention_args_ok("dense_attention_backward (gradients)", ld_grad, N, M, heads, depth);
  if (rc != DSPH_OK) return rc;
  if (!aligned16({q, k, v, out, dout, dq, dk, dv})) {
    set_error("dense_attention_backward: q, k, v, out, dout, dq, dk and dv must be 16-byte aligned");
    return DSPH_E_BADARG;
  }
  DeviceGuard guard(device);
  if (N <= 0 || M <= 0) return DSPH_OK;
  int64_t nblk;
  unsigned grid;
  rc = dense_grid("dense_attention_backward", N, M, heads, &nblk, &grid);
  if (rc != DSPH_OK) return rc;
  const float scale = (float)(1.0 / std::sqrt((double)depth));
  hipStream_t stream = (hipStream_t)hip_stream;
#define DENSE_BWD(DD)                                                                                                                  \
  hipLaunchKernelGGL(dense_attention_dq_kernel<DD>, dim3(grid), dim3(256), 0, stream, q, k, v, ld, out, lse, dout, delta, dq, ld_grad, M, \
                     (int)heads, nblk, scale);                                                                             \
  hipLaunchKernelGGL(dense_attention_dkv_kernel<DD>, dim3(grid), dim3(256), 0, stream, q, k, v, ld, lse, dout, delta, dk, dv, ld_grad, M, \
                     (int)heads, nblk, scale)
  DENSE_BY_DEPTH(depth, DENSE_BWD)
#undef DENSE_BWD
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

}  // extern "C"
