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
// The three kernels here are written once, over an arithmetic policy A that owns everything in which the exact-fp32 kernels
// (DaFp32, dense_attention.hip) and the bf16 split ones (DaSplit, dense_attention_split.hip) differ:
//   A::D, A::TS, A::NSUB, A::CB     depth, rows of a streamed tile, its 16-row sub-tiles, 16-channel blocks of an accumulator
//   A::Own, load_own, out_dot       an owned row as the B operand of the first product; its partial dout . out.  load_own gets
//                                   the row both ways, nullptr and own = false past M: fp32 branches on the flag, the split
//                                   on the pointer, as the code each was tuned with did (registers and schedule depend on it)
//   A::Stage, stage_load / _store   a thread's registers of a tile in flight: global -> registers -> LDS (the tile by pointer)
//   A::Tile<IMG>                    the LDS images of a tile that a kernel asks for: DA_ROW feeds the first product (tile_dot),
//                                   DA_TR the second (one padded float tile serves both in fp32; bf16 planes per image in the split)
//   A::Sink                         the second product: push(sub, x) where a sub-tile's P or dS exists, flush() after the tile --
//                                   fp32 issues its MFMAs in push, the split keeps the registers and multiplies in flush, so each
//                                   arithmetic compiles from its own schedule (fp32 dq with one multiply per tile costs a wave)
//   store_acc                       an accumulator, scaled, to its row
// and over MASKED, whose three decisions -- how a row's statistic is loaded, stored, and turned back into a probability -- are
// DaStat<MASKED> (dense_attention_common.h); the mask operand is a trailing parameter pack `MK... mk`, one DaMask when MASKED,
// nothing otherwise, so the unmasked instantiations keep the kernel arguments they had before there was a mask.
//
// A workgroup (4 waves) owns DA_TILE = 64 rows of one (map, head), a wave 16 of them, and streams the other side through LDS in
// tiles of TS rows; the next tile's global loads are in flight while the current one is computed.  The products are taken
// TRANSPOSED: S^T = T O^T with the streamed rows T (from LDS) as the A operand and the owned rows O (a register fragment, loaded
// once) as B, so a lane holds s[r] = S(tile row 16 sub + 4 (lane / 16) + r, owned row lane % 16).  That is, register by register,
// the B operand of the second product acc^T += T'^T X^T (X = P or dS; T' = the V, K, Q or dout tile) -- the A operand is read from
// LDS under the matching permutation -- so the softmax feeds the second MFMA without passing through LDS.  The statistics of an
// owned row live in its lane: a maximum / sum over a tile is one over its registers and the 4 lane groups (two xor shuffles).
// Tails: rows past M of a streamed tile are zero-filled and their logits masked (p = 0); owned rows past M compute on zeros and
// store nothing.
//
// Backward, no atomics, bitwise reproducible.  With delta_i,h = dout_i,h . out_i,h and p_ij = exp(s_ij - lse_i):
//   pass 1, query blocks, over key tiles:    ds_ij = p_ij (dout_i . v_j - delta_i)    dq_i = scale sum_j ds_ij k_j     (writes delta)
//   pass 2, key blocks, over query tiles:    dv_j = sum_i p_ij dout_i                 dk_j = scale sum_i ds_ij q_i
// Two launches on the caller's stream; every output element has one writer and a fixed order of summation.
#pragma once

#include "dense_attention_common.h"

namespace dsph {

typedef float da_f32x4 __attribute__((ext_vector_type(4)));

enum { DA_ROW = 1, DA_TR = 2 };  // the images of a tile: operand of the first product, of the second

__device__ __forceinline__ void da_lds4(float (&f)[4], const float* p) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  f[0] = t.x; f[1] = t.y; f[2] = t.z; f[3] = t.w;
}

template <class A, bool MASKED = false, typename... MK>
__global__ __launch_bounds__(256) void dense_attention_forward_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                       const float* __restrict__ v, int64_t ld, float* __restrict__ out,
                                                                       float* __restrict__ lse, int64_t M, int heads, int64_t nblk,
                                                                       float scale, MK... mk) {
  constexpr int D = A::D, TS = A::TS;
  using St = DaStat<MASKED>;
  __shared__ typename A::template Tile<DA_ROW> sk;
  __shared__ typename A::template Tile<DA_TR> sv;
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
  const DaBlock B = da_block(M, heads, D, nblk);
  typename A::Own qf;
  A::load_own(qf, B.own ? q + (B.base + B.row) * ld + B.ch : nullptr, B.own, g);
  da_f32x4 acc[A::CB];
#pragma unroll
  for (int b = 0; b < A::CB; ++b) acc[b] = da_f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -__builtin_huge_valf(), l = 0.f;
  const float* mrow = nullptr;
  if constexpr (MASKED) mrow = da_mask_row(da_mask_of(mk...), B, M);
  const int64_t ntiles = (M + TS - 1) / TS;
  typename A::Stage pk, pv;
  {
    const int valid = (int)(M < TS ? M : TS);
    A::stage_load(pk, k + B.base * ld + B.ch, ld, valid, tid);
    A::stage_load(pv, v + B.base * ld + B.ch, ld, valid, tid);
    A::stage_store(pk, &sk, tid);
    A::stage_store(pv, &sv, tid);
  }
  __syncthreads();
  for (int64_t t = 0; t < ntiles; ++t) {
    const int64_t j0 = t * TS;
    if (t + 1 < ntiles) {
      const int64_t left = M - (j0 + TS);
      const int valid = (int)(left < TS ? left : TS);
      A::stage_load(pk, k + (B.base + j0 + TS) * ld + B.ch, ld, valid, tid);
      A::stage_load(pv, v + (B.base + j0 + TS) * ld + B.ch, ld, valid, tid);
    }
    da_f32x4 s[A::NSUB];
    float mx = -__builtin_huge_valf();
#pragma unroll
    for (int sub = 0; sub < A::NSUB; ++sub) {
      float mb[4] = {0.f, 0.f, 0.f, 0.f};
      if constexpr (MASKED) da_mask_addend4(mb, mrow, j0 + 16 * sub + 4 * g, M);
      s[sub] = A::tile_dot(sk, sub, qf, lane);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[sub][r] = j0 + 16 * sub + 4 * g + r < M ? St::logit(s[sub][r], scale, mb[r]) : -__builtin_huge_valf();
        mx = fmaxf(mx, s[sub][r]);
      }
    }
    const float mn = fmaxf(m, da_group_max(mx));  // (finite: a tile holds at least one row below M)
    const float corr = __expf(m - mn);            // (first tile: m = -inf, corr = 0)
    float sum = 0.f;
#pragma unroll
    for (int sub = 0; sub < A::NSUB; ++sub)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[sub][r] = __expf(s[sub][r] - mn);
        sum += s[sub][r];
      }
    l = fmaf(l, corr, da_group_sum(sum));
    m = mn;
#pragma unroll
    for (int b = 0; b < A::CB; ++b) acc[b] *= corr;
    typename A::Sink pv_sink;  // (after the whole tile's softmax in both arithmetics: the rescaling above needs the tile's maximum)
#pragma unroll
    for (int sub = 0; sub < A::NSUB; ++sub) pv_sink.push(acc, sv, sub, s[sub], lane);
    pv_sink.flush(acc, sv, lane);
    __syncthreads();
    if (t + 1 < ntiles) {
      A::stage_store(pk, &sk, tid);
      A::stage_store(pv, &sv, tid);
    }
    __syncthreads();
  }
  if (!B.own) return;
  A::store_acc(out + (B.base + B.row) * ((int64_t)heads * D) + B.ch, acc, 1.f / l, g);
  if (lse != nullptr && g == 0) St::store(lse, B.base + B.row, heads, B.h, m, l);
}

// pass 1 of the backward: delta and dq of the owned query rows, over the key tiles
template <class A, bool MASKED = false, typename... MK>
__global__ __launch_bounds__(256) void dense_attention_dq_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                  const float* __restrict__ v, int64_t ld, const float* __restrict__ out,
                                                                  const float* __restrict__ lse, const float* __restrict__ dout,
                                                                  float* __restrict__ delta, float* __restrict__ dq, int64_t ldg, int64_t M,
                                                                  int heads, int64_t nblk, float scale,
                                                                  MK... mk) {
  constexpr int D = A::D, TS = A::TS;
  using St = DaStat<MASKED>;
  __shared__ typename A::template Tile<DA_ROW | DA_TR> sk;
  __shared__ typename A::template Tile<DA_ROW> sv;
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
  const DaBlock B = da_block(M, heads, D, nblk);
  const int64_t d = (int64_t)heads * D;
  typename A::Own qf, gf;
  float dl = 0.f;
  St st = {};  // of the owned row
  const float* mrow = nullptr;
  if constexpr (MASKED) mrow = da_mask_row(da_mask_of(mk...), B, M);
  A::load_own(qf, B.own ? q + (B.base + B.row) * ld + B.ch : nullptr, B.own, g);
  A::load_own(gf, B.own ? dout + (B.base + B.row) * d + B.ch : nullptr, B.own, g);
  if (B.own) {
    dl = A::out_dot(gf, out + (B.base + B.row) * d + B.ch, g);
    st = St::load(lse, (B.base + B.row) * heads + B.h);
  }
  dl = da_group_sum(dl);  // (the four lane groups of a row hold its D channels once)
  da_f32x4 acc[A::CB];
#pragma unroll
  for (int b = 0; b < A::CB; ++b) acc[b] = da_f32x4{0.f, 0.f, 0.f, 0.f};
  const int64_t ntiles = (M + TS - 1) / TS;
  typename A::Stage pk, pv;
  {
    const int valid = (int)(M < TS ? M : TS);
    A::stage_load(pk, k + B.base * ld + B.ch, ld, valid, tid);
    A::stage_load(pv, v + B.base * ld + B.ch, ld, valid, tid);
    A::stage_store(pk, &sk, tid);
    A::stage_store(pv, &sv, tid);
  }
  __syncthreads();
  for (int64_t t = 0; t < ntiles; ++t) {
    const int64_t j0 = t * TS;
    if (t + 1 < ntiles) {
      const int64_t left = M - (j0 + TS);
      const int valid = (int)(left < TS ? left : TS);
      A::stage_load(pk, k + (B.base + j0 + TS) * ld + B.ch, ld, valid, tid);
      A::stage_load(pv, v + (B.base + j0 + TS) * ld + B.ch, ld, valid, tid);
    }
    typename A::Sink dq_sink;
#pragma unroll
    for (int sub = 0; sub < A::NSUB; ++sub) {
      float mb[4] = {0.f, 0.f, 0.f, 0.f};
      if constexpr (MASKED) da_mask_addend4(mb, mrow, j0 + 16 * sub + 4 * g, M);
      const da_f32x4 s = A::tile_dot(sk, sub, qf, lane);
      const da_f32x4 dp = A::tile_dot(sv, sub, gf, lane);
      da_f32x4 ds;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = j0 + 16 * sub + 4 * g + r < M ? st.prob(s[r], scale, mb[r]) : 0.f;
        ds[r] = p * (dp[r] - dl);
      }
      dq_sink.push(acc, sk, sub, ds, lane);
    }
    dq_sink.flush(acc, sk, lane);
    __syncthreads();
    if (t + 1 < ntiles) {
      A::stage_store(pk, &sk, tid);
      A::stage_store(pv, &sv, tid);
    }
    __syncthreads();
  }
  if (!B.own) return;
  if (g == 0) delta[(B.base + B.row) * heads + B.h] = dl;
  A::store_acc(dq + (B.base + B.row) * ldg + B.ch, acc, scale, g);
}

// pass 2: dk and dv of the owned key rows, over the query tiles (q and dout rows in LDS, their statistic and delta beside them:
// sl holds component c of tile row t at c TS + t)
template <class A, bool MASKED = false, typename... MK>
__global__ __launch_bounds__(256) void dense_attention_dkv_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                   const float* __restrict__ v, int64_t ld, const float* __restrict__ lse,
                                                                   const float* __restrict__ dout, const float* __restrict__ delta,
                                                                   float* __restrict__ dk, float* __restrict__ dv, int64_t ldg, int64_t M,
                                                                   int heads, int64_t nblk, float scale,
                                                                   MK... mk) {
  constexpr int D = A::D, TS = A::TS;
  using St = DaStat<MASKED>;
  __shared__ typename A::template Tile<DA_ROW | DA_TR> sq;
  __shared__ typename A::template Tile<DA_ROW | DA_TR> sg;
  __shared__ __attribute__((aligned(16))) float sl[St::FLOATS * TS];
  __shared__ __attribute__((aligned(16))) float sd[TS];
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
  const DaBlock B = da_block(M, heads, D, nblk);
  const int64_t d = (int64_t)heads * D;
  typename A::Own kf, vf;
  A::load_own(kf, B.own ? k + (B.base + B.row) * ld + B.ch : nullptr, B.own, g);
  A::load_own(vf, B.own ? v + (B.base + B.row) * ld + B.ch : nullptr, B.own, g);
  da_f32x4 ak[A::CB], av[A::CB];
#pragma unroll
  for (int b = 0; b < A::CB; ++b) ak[b] = av[b] = da_f32x4{0.f, 0.f, 0.f, 0.f};
  const int64_t ntiles = (M + TS - 1) / TS;
  typename A::Stage pq, pg;
  St pst = {};  // threads 0..TS-1: statistic and delta of tile row tid
  float pd = 0.f;
  DaKeyMask km;
  if constexpr (MASKED) km = da_key_mask(da_mask_of(mk...), B, M);
  {
    const int valid = (int)(M < TS ? M : TS);
    A::stage_load(pq, q + B.base * ld + B.ch, ld, valid, tid);
    A::stage_load(pg, dout + B.base * d + B.ch, d, valid, tid);
    if (tid < valid) {
      const int64_t i = (B.base + tid) * heads + B.h;
      pst = St::load(lse, i);
      pd = delta[i];
    }
    A::stage_store(pq, &sq, tid);
    A::stage_store(pg, &sg, tid);
    if (tid < TS) {
      sl[tid] = pst.f[0]; sd[tid] = pd;
#pragma unroll
      for (int c = 1; c < St::FLOATS; ++c) sl[c * TS + tid] = pst.f[c];
    }
  }
  __syncthreads();
  for (int64_t t = 0; t < ntiles; ++t) {
    const int64_t i0 = t * TS;
    if (t + 1 < ntiles) {
      const int64_t left = M - (i0 + TS);
      const int valid = (int)(left < TS ? left : TS);
      A::stage_load(pq, q + (B.base + i0 + TS) * ld + B.ch, ld, valid, tid);
      A::stage_load(pg, dout + (B.base + i0 + TS) * d + B.ch, d, valid, tid);
      pst = {};
      pd = 0.f;
      if (tid < valid) {
        const int64_t i = (B.base + i0 + TS + tid) * heads + B.h;
        pst = St::load(lse, i);
        pd = delta[i];
      }
    }
    typename A::Sink dv_sink, dk_sink;
#pragma unroll
    for (int sub = 0; sub < A::NSUB; ++sub) {
      const da_f32x4 s = A::tile_dot(sq, sub, kf, lane);   // s[r]: query i0 + 16 sub + 4 g + r, the lane's key
      const da_f32x4 dp = A::tile_dot(sg, sub, vf, lane);
      float lq[St::FLOATS][4], dq4[4], mb[4] = {0.f, 0.f, 0.f, 0.f};
      da_lds4(lq[0], sl + 16 * sub + 4 * g);
      da_lds4(dq4, sd + 16 * sub + 4 * g);
      if constexpr (MASKED) da_key_mask_addend4(mb, km, i0 + 16 * sub + 4 * g, M);
#pragma unroll
      for (int c = 1; c < St::FLOATS; ++c) da_lds4(lq[c], sl + c * TS + 16 * sub + 4 * g);
      da_f32x4 p, ds;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        St st;
#pragma unroll
        for (int c = 0; c < St::FLOATS; ++c) st.f[c] = lq[c][r];
        p[r] = i0 + 16 * sub + 4 * g + r < M ? st.prob(s[r], scale, mb[r]) : 0.f;
        ds[r] = p[r] * (dp[r] - dq4[r]);
      }
      dv_sink.push(av, sg, sub, p, lane);
      dk_sink.push(ak, sq, sub, ds, lane);
    }
    dv_sink.flush(av, sg, lane);
    dk_sink.flush(ak, sq, lane);
    __syncthreads();
    if (t + 1 < ntiles) {
      A::stage_store(pq, &sq, tid);
      A::stage_store(pg, &sg, tid);
      if (tid < TS) {
        sl[tid] = pst.f[0]; sd[tid] = pd;
#pragma unroll
        for (int c = 1; c < St::FLOATS; ++c) sl[c * TS + tid] = pst.f[c];
      }
    }
    __syncthreads();
  }
  if (!B.own) return;
  A::store_acc(dv + (B.base + B.row) * ldg + B.ch, av, 1.f, g);
  A::store_acc(dk + (B.base + B.row) * ldg + B.ch, ak, scale, g);
}

// The launches of a checked call with its policies chosen: <A, MASKED> from whether the call carries a mask.
template <class A>
void dense_launch_forward(const DenseCall& c) {
  if (c.mk.p != nullptr)
    hipLaunchKernelGGL((dense_attention_forward_kernel<A, true, DaMask>), dim3(c.grid), dim3(256), 0, c.stream, c.q, c.k, c.v, c.ld, c.out, c.stat,
                       c.M, (int)c.heads, c.nblk, c.scale, c.mk);
  else
    hipLaunchKernelGGL((dense_attention_forward_kernel<A>), dim3(c.grid), dim3(256), 0, c.stream, c.q, c.k, c.v, c.ld, c.out, c.stat, c.M,
                       (int)c.heads, c.nblk, c.scale);
}

template <class ADQ, class ADKV>
void dense_launch_backward(const DenseCall& c) {
  const float *out = c.out, *stat = c.stat;
  if (c.mk.p != nullptr) {
    hipLaunchKernelGGL((dense_attention_dq_kernel<ADQ, true, DaMask>), dim3(c.grid), dim3(256), 0, c.stream, c.q, c.k, c.v, c.ld, out, stat, c.dout,
                       c.delta, c.dq, c.ld_grad, c.M, (int)c.heads, c.nblk, c.scale, c.mk);
    hipLaunchKernelGGL((dense_attention_dkv_kernel<ADKV, true, DaMask>), dim3(c.grid), dim3(256), 0, c.stream, c.q, c.k, c.v, c.ld, stat, c.dout,
                       c.delta, c.dk, c.dv, c.ld_grad, c.M, (int)c.heads, c.nblk, c.scale, c.mk);
  } else {
    hipLaunchKernelGGL((dense_attention_dq_kernel<ADQ>), dim3(c.grid), dim3(256), 0, c.stream, c.q, c.k, c.v, c.ld, out, stat, c.dout, c.delta,
                       c.dq, c.ld_grad, c.M, (int)c.heads, c.nblk, c.scale);
    hipLaunchKernelGGL((dense_attention_dkv_kernel<ADKV>), dim3(c.grid), dim3(256), 0, c.stream, c.q, c.k, c.v, c.ld, stat, c.dout, c.delta,
                       c.dk, c.dv, c.ld_grad, c.M, (int)c.heads, c.nblk, c.scale);
  }
}

}  // namespace dsph
