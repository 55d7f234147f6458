// Dense attention on the bf16 matrix pipe: the kernels of dense_attention.hip (same blocking, same contract, same outputs) with every
// product on v_mfma_f32_16x16x32_bf16 through a split of its fp32 operands, fp32 accumulation:
//   DSPH_PREC_BF16X3   a = hi + lo         products hh + hl + lh                     (2^-16 relative per operand)
//   DSPH_PREC_BF16X6   a = hi + mid + lo   products hh + hm + mh + hl + lh + mm      (fp32-equivalent)
// Each term is the round-to-nearest bf16 of the running remainder (a - hi and a - hi - mid are exact in fp32); bf16 has fp32's
// exponent range, so there is no scale rule.  The softmax statistics, exp, lse, delta and every rescaling stay fp32 on the vector unit.
// Depths 32 and 64: the contraction of the first product is one or two full K = 32 steps.
//
// A workgroup (4 waves) owns 64 rows of one (map, head), a wave 16, and streams the other side through LDS in tiles of TS rows
// (64; 32 where the images of a 64-row tile pass 64 KiB: the six-term backward and the three-term dk / dv at depth 64), the
// next tile's global loads in flight.  A tile is split ONCE, at staging, into bf16 planes per term, in up to two images:
//   row image  [term][TS][D]       the A operand of the first product  S^T = T O^T  (T the tile, O the owned rows, split once into
//                                  registers as the B operand): lane l reads channels 32 ks + 8 (l / 16) + j, j = 0..7, of tile
//                                  row 16 sub + l % 16 -- 16 bytes, conflict-free under the chunk swizzle of das_off.
//   transposed [term][D][TS]       the A operand of the second product  acc^T += T'^T X^T  (X = P or dS), which sums over tile
//                                  rows.  The first product leaves lane l with S(tile row 16 sub + 4 g + r, owned row l % 16),
//                                  g = l / 16, in register r of sub-tile sub; the B operand of 16x16x32 wants k = 8 g + j, j = 0..7,
//                                  for column l % 16.  So step u of the second product takes the sub-tiles 2 u and 2 u + 1: its
//                                  element j is register j % 4 of sub-tile 2 u + j / 4, i.e. k = 8 g + j is tile row
//                                  16 (2 u + j / 4) + 4 g + j % 4, and the softmax feeds the MFMA from registers, no LDS.  The
//                                  image stores tile row t at position 32 u + 8 g + 4 (j / 4) + j % 4 of its channel (das_pos),
//                                  which makes the A operand -- channel 16 b + l % 16, those eight rows -- 16 contiguous bytes.
// P and dS are split per element in registers.  Tails as in the fp32 kernels: rows past M of a tile are zero and their
// probabilities masked; owned rows past M compute on zeros and store nothing.  No atomics, one writer per element.
#include <cmath>

#include "dense_attention_common.h"

namespace dsph {

typedef float das_f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 das_bf16x8 __attribute__((ext_vector_type(8)));

__host__ __device__ constexpr int das_terms(int prec) { return prec == DSPH_PREC_BF16X3 ? 2 : 3; }

template <int D, int TS>
struct DasShape {
  static_assert((D == 32 || D == 64) && (TS == 32 || TS == 64), "depths 32 and 64, tiles of 32 or 64 rows");
  static constexpr int KS = D / 32;             // K = 32 steps of the first product
  static constexpr int CB = D / 16;             // 16-channel blocks of the accumulator
  static constexpr int NSUB = TS / 16;          // 16-row sub-tiles of a tile
  static constexpr int NU = TS / 32;            // K = 32 steps of the second product
  static constexpr int ROWIMG = TS * D;         // bf16 of one term's plane, row image [TS][D] and transposed image [D][TS]
  static constexpr int TRIMG = D * TS;
  static constexpr int RPT = TS * (D / 4) / 256;  // staging: a thread holds 4 channels of RPT neighbouring rows
  static_assert(RPT == 2 || RPT == 4, "a thread packs 2 or 4 rows of a channel into one transposed store");
};

// bytes of LDS of a kernel (0 forward, 1 dq, 2 dk / dv) with tiles of ts rows; the tile is 64 rows where that fits 64 KiB
__host__ __device__ constexpr int das_lds_bytes(int kind, int d, int ts, int nt) {
  const int row = ts * d * 2, tr = d * ts * 2;
  return kind == 0 ? nt * (row + tr) : (kind == 1 ? nt * (2 * row + tr) : nt * 2 * (row + tr) + 2 * ts * 4);
}
__host__ __device__ constexpr int das_tile_rows(int kind, int d, int nt) { return das_lds_bytes(kind, d, 64, nt) <= 64 * 1024 ? 64 : 32; }

template <int NT>
struct DasFrag {
  das_bf16x8 t[NT];  // hi, lo / hi, mid, lo
};

// a = t[0] + t[1] (+ t[2]) + what is left: each term the nearest bf16 of the running remainder
template <int NT>
__device__ __forceinline__ void das_split1(float a, __bf16 (&t)[NT]) {
  t[0] = (__bf16)a;
  float r = a - (float)t[0];
  t[1] = (__bf16)r;
  if constexpr (NT == 3) {
    r -= (float)t[1];
    t[2] = (__bf16)r;
  }
}

template <int NT>
__device__ __forceinline__ DasFrag<NT> das_split8(const float (&v)[8]) {
  DasFrag<NT> f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    __bf16 t[NT];
    das_split1<NT>(v[j], t);
#pragma unroll
    for (int i = 0; i < NT; ++i) f.t[i][j] = t[i];
  }
  return f;
}

// c += A B over the listed partial products, small terms first
template <int NT>
__device__ __forceinline__ das_f32x4 das_mfma(const DasFrag<NT>& a, const DasFrag<NT>& b, das_f32x4 c) {
  if constexpr (NT == 3) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.t[0], b.t[2], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.t[2], b.t[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.t[1], b.t[1], c, 0, 0, 0);
  }
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.t[0], b.t[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.t[1], b.t[0], c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.t[0], b.t[0], c, 0, 0, 0);
}

// the owned row's B operand of the first product: step ks holds channels 32 ks + 8 g + j (row == nullptr: a row past M, zeros)
template <int D, int NT>
__device__ __forceinline__ void das_load_own(DasFrag<NT> (&f)[D / 32], float (&raw)[D / 32][8], const float* row, int g) {
#pragma unroll
  for (int ks = 0; ks < D / 32; ++ks) {
    float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
    if (row != nullptr) {
      lo = *reinterpret_cast<const float4*>(row + 32 * ks + 8 * g);
      hi = *reinterpret_cast<const float4*>(row + 32 * ks + 8 * g + 4);
    }
    raw[ks][0] = lo.x; raw[ks][1] = lo.y; raw[ks][2] = lo.z; raw[ks][3] = lo.w;
    raw[ks][4] = hi.x; raw[ks][5] = hi.y; raw[ks][6] = hi.z; raw[ks][7] = hi.w;
    f[ks] = das_split8<NT>(raw[ks]);
  }
}

// Offset of element (row, col) of an image with rows of W = 32 or 64 bf16.  Both products read an image as 16 rows x 16-byte
// chunks (chunk = 4 step + lane / 16).  A 16-byte LDS read is served in four groups of 16 lanes -- {0-3, 12-15, 20-27},
// {4-11, 16-19, 28-31} and the same plus 32 -- that is, eight rows with one chunk index and the other eight with the next, and a
// group is conflict-free when its 16 chunks fall on 16 different 16-byte bank groups of the 256 bytes LDS serves per cycle.  Plain
// rows of 64 or 128 bytes put them on 4 or 2; the chunk index is therefore xor-ed with a function of the row that is one-to-one
// on each such group: (row / 2) % 8 for 128-byte rows (two rows per 256 bytes), {0, 3, 2, 1}[(row / 4) % 4] for 64-byte rows.
template <int W>
__device__ __forceinline__ int das_off(int row, int col) {
  static_assert(W == 32 || W == 64, "rows of 64 or 128 bytes");
  const int swz = W == 64 ? (row >> 1) & 7 : (4 - ((row >> 2) & 3)) & 3;
  return row * W + ((((col >> 3) ^ swz) << 3) | (col & 7));
}

// c[r] = (row 16 sub + 4 g + r of the tile) . (the owned row of lane % 16), from the tile's row image
template <int D, int TS, int NT>
__device__ __forceinline__ das_f32x4 das_tile_dot(const __bf16* img, int sub, const DasFrag<NT> (&own)[D / 32], int lane) {
  using S = DasShape<D, TS>;
  das_f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < S::KS; ++ks) {
    const __bf16* p = img + das_off<D>(16 * sub + (lane & 15), 32 * ks + 8 * (lane >> 4));
    DasFrag<NT> a;
#pragma unroll
    for (int i = 0; i < NT; ++i) a.t[i] = *reinterpret_cast<const das_bf16x8*>(p + i * S::ROWIMG);
    c = das_mfma<NT>(a, own[ks], c);
  }
  return c;
}

// acc[b][r'] (channel 16 b + 4 g + r', owned row lane % 16) += sum over the tile rows t of tile[t][channel] x(t), x[sub][r] being
// what das_tile_dot returned for sub-tile sub, after the softmax; from the tile's transposed image
template <int D, int TS, int NT>
__device__ __forceinline__ void das_tile_acc(das_f32x4 (&acc)[D / 16], const __bf16* img, const das_f32x4 (&x)[TS / 16], int lane) {
  using S = DasShape<D, TS>;
#pragma unroll
  for (int u = 0; u < S::NU; ++u) {
    const float xv[8] = {x[2 * u][0], x[2 * u][1], x[2 * u][2], x[2 * u][3], x[2 * u + 1][0], x[2 * u + 1][1], x[2 * u + 1][2], x[2 * u + 1][3]};
    const DasFrag<NT> xb = das_split8<NT>(xv);
#pragma unroll
    for (int b = 0; b < S::CB; ++b) {
      const __bf16* p = img + das_off<TS>(16 * b + (lane & 15), 32 * u + 8 * (lane >> 4));
      DasFrag<NT> a;
#pragma unroll
      for (int i = 0; i < NT; ++i) a.t[i] = *reinterpret_cast<const das_bf16x8*>(p + i * S::TRIMG);
      acc[b] = das_mfma<NT>(a, xb, acc[b]);
    }
  }
}

// position of tile row t in a channel of the transposed image
__device__ __forceinline__ int das_pos(int t) { return (t & ~31) | ((t & 12) << 1) | ((t & 16) >> 2) | (t & 3); }

// staging: thread tid holds channels [4 c4, 4 c4 + 4) of the rows RPT a + i, c4 = tid % (D / 4), a = tid / (D / 4).
// global -> registers (zeros past `valid`)
template <int D, int TS, int RPT>
__device__ __forceinline__ void das_stage_load(float4 (&s)[RPT], const float* __restrict__ src, int64_t ld, int valid, int tid) {
  static_assert(RPT == DasShape<D, TS>::RPT, "the thread's rows of a tile");
  const int c4 = tid % (D / 4), r0 = tid / (D / 4) * RPT;
#pragma unroll
  for (int i = 0; i < RPT; ++i)
    s[i] = r0 + i < valid ? *reinterpret_cast<const float4*>(src + (r0 + i) * ld + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// registers -> the split planes of the row image (rimg) and / or the transposed image (timg); nullptr: the kernel has no such image
template <int D, int TS, int NT, int RPT>
__device__ __forceinline__ void das_stage_store(const float4 (&s)[RPT], __bf16* rimg, __bf16* timg, int tid) {
  using S = DasShape<D, TS>;
  static_assert(RPT == S::RPT, "the thread's rows of a tile");
  typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
  typedef __bf16 bf16xr __attribute__((ext_vector_type(RPT)));
  const int c4 = tid % (D / 4), r0 = tid / (D / 4) * RPT;
  __bf16 t[RPT][4][NT];
#pragma unroll
  for (int i = 0; i < RPT; ++i) {
    das_split1<NT>(s[i].x, t[i][0]);
    das_split1<NT>(s[i].y, t[i][1]);
    das_split1<NT>(s[i].z, t[i][2]);
    das_split1<NT>(s[i].w, t[i][3]);
  }
  if (rimg != nullptr) {
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int i = 0; i < RPT; ++i)
        *reinterpret_cast<bf16x4*>(rimg + n * S::ROWIMG + das_off<D>(r0 + i, 4 * c4)) = bf16x4{t[i][0][n], t[i][1][n], t[i][2][n], t[i][3][n]};
  }
  if (timg != nullptr) {
    const int pos = das_pos(r0);  // (RPT neighbouring rows from a multiple of RPT on: neighbouring positions)
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        bf16xr v;
#pragma unroll
        for (int i = 0; i < RPT; ++i) v[i] = t[i][c][n];
        *reinterpret_cast<bf16xr*>(timg + n * S::TRIMG + das_off<TS>(4 * c4 + c, pos)) = v;
      }
  }
}

// the lane's accumulator, times f, to channels [16 b + 4 g, + 4) of its row
template <int D>
__device__ __forceinline__ void das_store_acc(float* rowp, const das_f32x4 (&acc)[D / 16], float f, int g) {
#pragma unroll
  for (int b = 0; b < D / 16; ++b)
    *reinterpret_cast<float4*>(rowp + 16 * b + 4 * g) = make_float4(acc[b][0] * f, acc[b][1] * f, acc[b][2] * f, acc[b][3] * f);
}

// MASKED, here and below: as in dense_attention.hip -- the mask's addend goes onto the fp32 logit after the product (it is never
// split) and `lse` is the pair buffer (N, M, heads, 2) = (m, log l).
template <int D, int PREC, bool MASKED = false, typename... MK>
__global__ __launch_bounds__(256) void dense_attention_split_forward_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                             const float* __restrict__ v, int64_t ld, float* __restrict__ out,
                                                                             float* __restrict__ lse, int64_t M, int heads, int64_t nblk,
                                                                             float scale, MK... mk) {
  constexpr int NT = das_terms(PREC), TS = das_tile_rows(0, D, NT);
  using S = DasShape<D, TS>;
  __shared__ __attribute__((aligned(16))) __bf16 sk[NT * S::ROWIMG];
  __shared__ __attribute__((aligned(16))) __bf16 sv[NT * S::TRIMG];
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
  const DaBlock B = da_block(M, heads, D, nblk);
  DasFrag<NT> qf[S::KS];
  {
    float raw[S::KS][8];
    das_load_own<D, NT>(qf, raw, B.own ? q + (B.base + B.row) * ld + B.ch : nullptr, g);
  }
  das_f32x4 acc[S::CB];
#pragma unroll
  for (int b = 0; b < S::CB; ++b) acc[b] = das_f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -__builtin_huge_valf(), l = 0.f;
  const float* mrow = nullptr;
  if constexpr (MASKED) mrow = da_mask_row(da_mask_of(mk...), B, M);
  const int64_t ntiles = (M + TS - 1) / TS;
  float4 pk[S::RPT], pv[S::RPT];
  {
    const int valid = (int)(M < TS ? M : TS);
    das_stage_load<D, TS, S::RPT>(pk, k + B.base * ld + B.ch, ld, valid, tid);
    das_stage_load<D, TS, S::RPT>(pv, v + B.base * ld + B.ch, ld, valid, tid);
    das_stage_store<D, TS, NT, S::RPT>(pk, sk, nullptr, tid);
    das_stage_store<D, TS, NT, S::RPT>(pv, nullptr, sv, tid);
  }
  __syncthreads();
  for (int64_t t = 0; t < ntiles; ++t) {
    const int64_t j0 = t * TS;
    if (t + 1 < ntiles) {
      const int64_t left = M - (j0 + TS);
      const int valid = (int)(left < TS ? left : TS);
      das_stage_load<D, TS, S::RPT>(pk, k + (B.base + j0 + TS) * ld + B.ch, ld, valid, tid);
      das_stage_load<D, TS, S::RPT>(pv, v + (B.base + j0 + TS) * ld + B.ch, ld, valid, tid);
    }
    das_f32x4 s[S::NSUB];
    float mx = -__builtin_huge_valf();
#pragma unroll
    for (int sub = 0; sub < S::NSUB; ++sub) {
      float mb[4];
      if constexpr (MASKED) da_mask_addend4(mb, mrow, j0 + 16 * sub + 4 * g, M);
      s[sub] = das_tile_dot<D, TS, NT>(sk, sub, qf, lane);
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
    for (int sub = 0; sub < S::NSUB; ++sub)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[sub][r] = __expf(s[sub][r] - mn);
        sum += s[sub][r];
      }
    l = fmaf(l, corr, da_group_sum(sum));
    m = mn;
#pragma unroll
    for (int b = 0; b < S::CB; ++b) acc[b] *= corr;
    das_tile_acc<D, TS, NT>(acc, sv, s, lane);
    __syncthreads();
    if (t + 1 < ntiles) {
      das_stage_store<D, TS, NT, S::RPT>(pk, sk, nullptr, tid);
      das_stage_store<D, TS, NT, S::RPT>(pv, nullptr, sv, tid);
    }
    __syncthreads();
  }
  if (!B.own) return;
  das_store_acc<D>(out + (B.base + B.row) * ((int64_t)heads * D) + B.ch, acc, 1.f / l, g);
  if (lse != nullptr && g == 0) {
    if constexpr (MASKED) {
      *reinterpret_cast<float2*>(lse + 2 * ((B.base + B.row) * heads + B.h)) = make_float2(m, logf(l));
    } else {
      lse[(B.base + B.row) * heads + B.h] = m + logf(l);
    }
  }
}

// pass 1 of the backward: delta and dq of the owned query rows, over the key tiles
template <int D, int PREC, bool MASKED = false, typename... MK>
__global__ __launch_bounds__(256) void dense_attention_split_dq_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                        const float* __restrict__ v, int64_t ld, const float* __restrict__ out,
                                                                        const float* __restrict__ lse, const float* __restrict__ dout,
                                                                        float* __restrict__ delta, float* __restrict__ dq, int64_t ldg, int64_t M,
                                                                        int heads, int64_t nblk, float scale,
                                                                        MK... mk) {
  constexpr int NT = das_terms(PREC), TS = das_tile_rows(1, D, NT);
  using S = DasShape<D, TS>;
  __shared__ __attribute__((aligned(16))) __bf16 sk[NT * S::ROWIMG];
  __shared__ __attribute__((aligned(16))) __bf16 skt[NT * S::TRIMG];
  __shared__ __attribute__((aligned(16))) __bf16 sv[NT * S::ROWIMG];
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
  const DaBlock B = da_block(M, heads, D, nblk);
  const int64_t d = (int64_t)heads * D;
  DasFrag<NT> qf[S::KS], gf[S::KS];
  float dl = 0.f, ls = 0.f;
  float ll = 0.f;  // MASKED: (ls, ll) = (m, log l) of the owned row
  const float* mrow = nullptr;
  if constexpr (MASKED) mrow = da_mask_row(da_mask_of(mk...), B, M);
  {
    float raw[S::KS][8], graw[S::KS][8];
    das_load_own<D, NT>(qf, raw, B.own ? q + (B.base + B.row) * ld + B.ch : nullptr, g);
    das_load_own<D, NT>(gf, graw, B.own ? dout + (B.base + B.row) * d + B.ch : nullptr, g);
    if (B.own) {
      const float* orow = out + (B.base + B.row) * d + B.ch;
#pragma unroll
      for (int ks = 0; ks < S::KS; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) dl = fmaf(graw[ks][j], orow[32 * ks + 8 * g + j], dl);
      if constexpr (MASKED) {
        const float2 st = *reinterpret_cast<const float2*>(lse + 2 * ((B.base + B.row) * heads + B.h));
        ls = st.x; ll = st.y;
      } else {
        ls = lse[(B.base + B.row) * heads + B.h];
      }
    }
  }
  dl = da_group_sum(dl);  // (the four lane groups of a row hold its D channels once)
  das_f32x4 acc[S::CB];
#pragma unroll
  for (int b = 0; b < S::CB; ++b) acc[b] = das_f32x4{0.f, 0.f, 0.f, 0.f};
  const int64_t ntiles = (M + TS - 1) / TS;
  float4 pk[S::RPT], pv[S::RPT];
  {
    const int valid = (int)(M < TS ? M : TS);
    das_stage_load<D, TS, S::RPT>(pk, k + B.base * ld + B.ch, ld, valid, tid);
    das_stage_load<D, TS, S::RPT>(pv, v + B.base * ld + B.ch, ld, valid, tid);
    das_stage_store<D, TS, NT, S::RPT>(pk, sk, skt, tid);
    das_stage_store<D, TS, NT, S::RPT>(pv, sv, nullptr, tid);
  }
  __syncthreads();
  for (int64_t t = 0; t < ntiles; ++t) {
    const int64_t j0 = t * TS;
    if (t + 1 < ntiles) {
      const int64_t left = M - (j0 + TS);
      const int valid = (int)(left < TS ? left : TS);
      das_stage_load<D, TS, S::RPT>(pk, k + (B.base + j0 + TS) * ld + B.ch, ld, valid, tid);
      das_stage_load<D, TS, S::RPT>(pv, v + (B.base + j0 + TS) * ld + B.ch, ld, valid, tid);
    }
    das_f32x4 ds[S::NSUB];
#pragma unroll
    for (int sub = 0; sub < S::NSUB; ++sub) {
      float mb[4];
      if constexpr (MASKED) da_mask_addend4(mb, mrow, j0 + 16 * sub + 4 * g, M);
      const das_f32x4 s = das_tile_dot<D, TS, NT>(sk, sub, qf, lane);
      const das_f32x4 dp = das_tile_dot<D, TS, NT>(sv, sub, gf, lane);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float p;
        if constexpr (MASKED) {
          p = j0 + 16 * sub + 4 * g + r < M ? __expf((da_masked_logit(s[r], scale, mb[r]) - ls) - ll) : 0.f;
        } else {
          p = j0 + 16 * sub + 4 * g + r < M ? __expf(fmaf(s[r], scale, -ls)) : 0.f;
        }
        ds[sub][r] = p * (dp[r] - dl);
      }
    }
    das_tile_acc<D, TS, NT>(acc, skt, ds, lane);
    __syncthreads();
    if (t + 1 < ntiles) {
      das_stage_store<D, TS, NT, S::RPT>(pk, sk, skt, tid);
      das_stage_store<D, TS, NT, S::RPT>(pv, sv, nullptr, tid);
    }
    __syncthreads();
  }
  if (!B.own) return;
  if (g == 0) delta[(B.base + B.row) * heads + B.h] = dl;
  das_store_acc<D>(dq + (B.base + B.row) * ldg + B.ch, acc, scale, g);
}

// pass 2: dk and dv of the owned key rows, over the query tiles (q and dout rows in LDS, their lse and delta beside them)
template <int D, int PREC, bool MASKED = false, typename... MK>
__global__ __launch_bounds__(256) void dense_attention_split_dkv_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                         const float* __restrict__ v, int64_t ld, const float* __restrict__ lse,
                                                                         const float* __restrict__ dout, const float* __restrict__ delta,
                                                                         float* __restrict__ dk, float* __restrict__ dv, int64_t ldg, int64_t M,
                                                                         int heads, int64_t nblk, float scale,
                                                                         MK... mk) {
  constexpr int NT = das_terms(PREC), TS = das_tile_rows(2, D, NT);
  using S = DasShape<D, TS>;
  constexpr int ST = MASKED ? 2 : 1;  // floats of a row's statistic: lse, or m and, TS further on, log l
  static_assert(das_lds_bytes(2, D, TS, NT) + (ST - 1) * TS * 4 <= 64 * 1024, "the second statistic keeps the tile rows das_tile_rows chose");
  __shared__ __attribute__((aligned(16))) __bf16 sq[NT * S::ROWIMG];
  __shared__ __attribute__((aligned(16))) __bf16 sqt[NT * S::TRIMG];
  __shared__ __attribute__((aligned(16))) __bf16 sg[NT * S::ROWIMG];
  __shared__ __attribute__((aligned(16))) __bf16 sgt[NT * S::TRIMG];
  __shared__ __attribute__((aligned(16))) float sl[ST * TS];
  __shared__ __attribute__((aligned(16))) float sd[TS];
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4;
  const DaBlock B = da_block(M, heads, D, nblk);
  const int64_t d = (int64_t)heads * D;
  DasFrag<NT> kf[S::KS], vf[S::KS];
  {
    float raw[S::KS][8];
    das_load_own<D, NT>(kf, raw, B.own ? k + (B.base + B.row) * ld + B.ch : nullptr, g);
    das_load_own<D, NT>(vf, raw, B.own ? v + (B.base + B.row) * ld + B.ch : nullptr, g);
  }
  das_f32x4 ak[S::CB], av[S::CB];
#pragma unroll
  for (int b = 0; b < S::CB; ++b) ak[b] = av[b] = das_f32x4{0.f, 0.f, 0.f, 0.f};
  const int64_t ntiles = (M + TS - 1) / TS;
  float4 pq[S::RPT], pg[S::RPT];
  float pl = 0.f, pd = 0.f;  // threads 0..TS-1: lse and delta of tile row tid
  float pl2 = 0.f;           // MASKED: (pl, pl2) = (m, log l)
  DaKeyMask km;
  if constexpr (MASKED) km = da_key_mask(da_mask_of(mk...), B, M);
  {
    const int valid = (int)(M < TS ? M : TS);
    das_stage_load<D, TS, S::RPT>(pq, q + B.base * ld + B.ch, ld, valid, tid);
    das_stage_load<D, TS, S::RPT>(pg, dout + B.base * d + B.ch, d, valid, tid);
    if (tid < valid) {
      if constexpr (MASKED) {
        const float2 st = *reinterpret_cast<const float2*>(lse + 2 * ((B.base + tid) * heads + B.h));
        pl = st.x; pl2 = st.y;
      } else {
        pl = lse[(B.base + tid) * heads + B.h];
      }
      pd = delta[(B.base + tid) * heads + B.h];
    }
    das_stage_store<D, TS, NT, S::RPT>(pq, sq, sqt, tid);
    das_stage_store<D, TS, NT, S::RPT>(pg, sg, sgt, tid);
    if (tid < TS) {
      sl[tid] = pl; sd[tid] = pd;
      if constexpr (MASKED) sl[TS + tid] = pl2;
    }
  }
  __syncthreads();
  for (int64_t t = 0; t < ntiles; ++t) {
    const int64_t i0 = t * TS;
    if (t + 1 < ntiles) {
      const int64_t left = M - (i0 + TS);
      const int valid = (int)(left < TS ? left : TS);
      das_stage_load<D, TS, S::RPT>(pq, q + (B.base + i0 + TS) * ld + B.ch, ld, valid, tid);
      das_stage_load<D, TS, S::RPT>(pg, dout + (B.base + i0 + TS) * d + B.ch, d, valid, tid);
      pl = pd = pl2 = 0.f;
      if (tid < valid) {
        if constexpr (MASKED) {
          const float2 st = *reinterpret_cast<const float2*>(lse + 2 * ((B.base + i0 + TS + tid) * heads + B.h));
          pl = st.x; pl2 = st.y;
        } else {
          pl = lse[(B.base + i0 + TS + tid) * heads + B.h];
        }
        pd = delta[(B.base + i0 + TS + tid) * heads + B.h];
      }
    }
    das_f32x4 p[S::NSUB], ds[S::NSUB];
#pragma unroll
    for (int sub = 0; sub < S::NSUB; ++sub) {
      const das_f32x4 s = das_tile_dot<D, TS, NT>(sq, sub, kf, lane);   // s[r]: query i0 + 16 sub + 4 g + r, the lane's key
      const das_f32x4 dp = das_tile_dot<D, TS, NT>(sg, sub, vf, lane);
      const float4 l4 = *reinterpret_cast<const float4*>(sl + 16 * sub + 4 * g);
      const float4 d4 = *reinterpret_cast<const float4*>(sd + 16 * sub + 4 * g);
      const float lq[4] = {l4.x, l4.y, l4.z, l4.w}, dq4[4] = {d4.x, d4.y, d4.z, d4.w};
      float mb[4], lq2[4];
      if constexpr (MASKED) {
        da_key_mask_addend4(mb, km, i0 + 16 * sub + 4 * g, M);
        const float4 t4 = *reinterpret_cast<const float4*>(sl + TS + 16 * sub + 4 * g);
        lq2[0] = t4.x; lq2[1] = t4.y; lq2[2] = t4.z; lq2[3] = t4.w;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if constexpr (MASKED) {
          p[sub][r] = i0 + 16 * sub + 4 * g + r < M ? __expf((da_masked_logit(s[r], scale, mb[r]) - lq[r]) - lq2[r]) : 0.f;
        } else {
          p[sub][r] = i0 + 16 * sub + 4 * g + r < M ? __expf(fmaf(s[r], scale, -lq[r])) : 0.f;
        }
        ds[sub][r] = p[sub][r] * (dp[r] - dq4[r]);
      }
    }
    das_tile_acc<D, TS, NT>(av, sgt, p, lane);
    das_tile_acc<D, TS, NT>(ak, sqt, ds, lane);
    __syncthreads();
    if (t + 1 < ntiles) {
      das_stage_store<D, TS, NT, S::RPT>(pq, sq, sqt, tid);
      das_stage_store<D, TS, NT, S::RPT>(pg, sg, sgt, tid);
      if (tid < TS) {
        sl[tid] = pl; sd[tid] = pd;
        if constexpr (MASKED) sl[TS + tid] = pl2;
      }
    }
    __syncthreads();
  }
  if (!B.own) return;
  das_store_acc<D>(dv + (B.base + B.row) * ldg + B.ch, av, 1.f, g);
  das_store_acc<D>(dk + (B.base + B.row) * ldg + B.ch, ak, scale, g);
}

// the precision code of a _prec entry point: DSPH_PREC_FP32 and the two splits; a split runs depths 32 and 64 only
static int dense_precision_ok(const char* who, int32_t precision, int32_t depth) {
  if (precision != DSPH_PREC_FP32 && precision != DSPH_PREC_BF16X6 && precision != DSPH_PREC_BF16X3) {
    set_error("%s: unknown precision code %d (DSPH_PREC_FP32, DSPH_PREC_BF16X6 or DSPH_PREC_BF16X3)", who, (int)precision);
    return DSPH_E_BADARG;
  }
  if (precision != DSPH_PREC_FP32 && depth != 32 && depth != 64) {
    set_error("%s: the bf16 split arithmetics run depths 32, 64 per head, not %d (DSPH_PREC_FP32 runs 4, 8, 16 too)", who, (int)depth);
    return DSPH_E_UNSUPPORTED;
  }
  return DSPH_OK;
}

// KERNEL<depth, precision> of a split call (depth 32 or 64, precision one of the two splits)
#define DENSE_SPLIT_DISPATCH(depth, precision, CALL)        \
  do {                                                      \
    if ((precision) == DSPH_PREC_BF16X6) {                  \
      if ((depth) == 32) { CALL(32, DSPH_PREC_BF16X6); }    \
      else { CALL(64, DSPH_PREC_BF16X6); }                  \
    } else {                                                \
      if ((depth) == 32) { CALL(32, DSPH_PREC_BF16X3); }    \
      else { CALL(64, DSPH_PREC_BF16X3); }                  \
    }                                                       \
  } while (0)

}  // namespace dsph

extern "C" {

int dsph_dense_attention_forward_prec(const float* q, const float* k, const float* v, int64_t ld, float* out, float* lse, int64_t N,
                                      int64_t M, int32_t heads, int32_t depth, int32_t precision, int device, void* hip_stream) {
  using namespace dsph;
  if (precision == DSPH_PREC_FP32) return dsph_dense_attention_forward(q, k, v, ld, out, lse, N, M, heads, depth, device, hip_stream);
  if (!q || !k || !v || !out) { set_error("dense_attention_forward: NULL pointer"); return DSPH_E_BADARG; }
  int rc = dense_attention_args_ok("dense_attention_forward", ld, N, M, heads, depth);
  if (rc == DSPH_OK) rc = dense_precision_ok("dense_attention_forward", precision, depth);
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
#define DENSE_FWD(DD, PP) \
  hipLaunchKernelGGL((dense_attention_split_forward_kernel<DD, PP>), dim3(grid), dim3(256), 0, stream, q, k, v, ld, out, lse, M, (int)heads, nblk, scale)
  DENSE_SPLIT_DISPATCH(depth, precision, DENSE_FWD);
#undef DENSE_FWD
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

int dsph_dense_attention_backward_prec(const float* q, const float* k, const float* v, int64_t ld, const float* out, const float* lse,
                                       const float* dout, float* delta, float* dq, float* dk, float* dv, int64_t ld_grad, int64_t N,
                                       int64_t M, int32_t heads, int32_t depth, int32_t precision, int device, void* hip_stream) {
  using namespace dsph;
  if (precision == DSPH_PREC_FP32)
    return dsph_dense_attention_backward(q, k, v, ld, out, lse, dout, delta, dq, dk, dv, ld_grad, N, M, heads, depth, device, hip_stream);
  if (!q || !k || !v || !out || !lse || !dout || !delta || !dq || !dk || !dv) {
    set_error("dense_attention_backward: NULL pointer");
    return DSPH_E_BADARG;
  }
  int rc = dense_attention_args_ok("dense_attention_backward", ld, N, M, heads, depth);
  if (rc == DSPH_OK) rc = dense_attention_args_ok("dense_attention_backward (gradients)", ld_grad, N, M, heads, depth);
  if (rc == DSPH_OK) rc = dense_precision_ok("dense_attention_backward", precision, depth);
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
#define DENSE_BWD(DD, PP)                                                                                                                       \
  hipLaunchKernelGGL((dense_attention_split_dq_kernel<DD, PP>), dim3(grid), dim3(256), 0, stream, q, k, v, ld, out, lse, dout, delta, dq, ld_grad, \
                     M, (int)heads, nblk, scale);                                                                                   \
  hipLaunchKernelGGL((dense_attention_split_dkv_kernel<DD, PP>), dim3(grid), dim3(256), 0, stream, q, k, v, ld, lse, dout, delta, dk, dv, ld_grad, \
                     M, (int)heads, nblk, scale)
  DENSE_SPLIT_DISPATCH(depth, precision, DENSE_BWD);
#undef DENSE_BWD
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

int dsph_dense_attention_forward_masked(const float* q, const float* k, const float* v, int64_t ld, float* out, float* stat, const float* mask,
                                        int64_t mask_stride_batch, int64_t mask_stride_head, int64_t mask_stride_query, int64_t N, int64_t M,
                                        int32_t heads, int32_t depth, int32_t precision, int device, void* hip_stream) {
  using namespace dsph;
  const char* who = "dense_attention_forward_masked";
  if (!q || !k || !v || !out) { set_error("%s: NULL pointer", who); return DSPH_E_BADARG; }
  int rc = dense_mask_args_ok(who, mask, mask_stride_batch, mask_stride_head, mask_stride_query);
  if (rc == DSPH_OK) rc = dense_attention_args_ok(who, ld, N, M, heads, depth);
  if (rc == DSPH_OK) rc = dense_precision_ok(who, precision, depth);
  if (rc != DSPH_OK) return rc;
  if (!aligned16({q, k, v, out}) || (reinterpret_cast<uintptr_t>(stat) & 7) != 0) {
    set_error("%s: q, k, v and out must be 16-byte aligned, stat 8-byte", who);
    return DSPH_E_BADARG;
  }
  DeviceGuard guard(device);
  if (N <= 0 || M <= 0) return DSPH_OK;
  const DaMask mk{mask, mask_stride_batch, mask_stride_head, mask_stride_query};
  hipStream_t stream = (hipStream_t)hip_stream;
  if (precision == DSPH_PREC_FP32) return dense_attention_forward_masked_fp32(q, k, v, ld, out, stat, mk, N, M, heads, depth, stream);
  int64_t nblk;
  unsigned grid;
  rc = dense_grid(who, N, M, heads, &nblk, &grid);
  if (rc != DSPH_OK) return rc;
  const float scale = (float)(1.0 / std::sqrt((double)depth));
#define DENSE_FWD(DD, PP)                                                                                                                      \
  hipLaunchKernelGGL((dense_attention_split_forward_kernel<DD, PP, true, DaMask>), dim3(grid), dim3(256), 0, stream, q, k, v, ld, out, stat, M, (int)heads, \
                     nblk, scale, mk)
  DENSE_SPLIT_DISPATCH(depth, precision, DENSE_FWD);
#undef DENSE_FWD
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

int dsph_dense_attention_backward_masked(const float* q, const float* k, const float* v, int64_t ld, const float* out, const float* stat,
                                         const float* mask, int64_t mask_stride_batch, int64_t mask_stride_head, int64_t mask_stride_query,
                                         const float* dout, float* delta, float* dq, float* dk, float* dv, int64_t ld_grad, int64_t N, int64_t M,
                                         int32_t heads, int32_t depth, int32_t precision, int device, void* hip_stream) {
  using namespace dsph;
  const char* who = "dense_attention_backward_masked";
  if (!q || !k || !v || !out || !stat || !dout || !delta || !dq || !dk || !dv) { set_error("%s: NULL pointer", who); return DSPH_E_BADARG; }
  int rc = dense_mask_args_ok(who, mask, mask_stride_batch, mask_stride_head, mask_stride_query);
  if (rc == DSPH_OK) rc = dense_attention_args_ok(who, ld, N, M, heads, depth);
  if (rc == DSPH_OK) rc = dense_attention_args_ok("dense_attention_backward_masked (gradients)", ld_grad, N, M, heads, depth);
  if (rc == DSPH_OK) rc = dense_precision_ok(who, precision, depth);
  if (rc != DSPH_OK) return rc;
  if (!aligned16({q, k, v, out, dout, dq, dk, dv}) || (reinterpret_cast<uintptr_t>(stat) & 7) != 0) {
    set_error("%s: q, k, v, out, dout, dq, dk and dv must be 16-byte aligned, stat 8-byte", who);
    return DSPH_E_BADARG;
  }
  DeviceGuard guard(device);
  if (N <= 0 || M <= 0) return DSPH_OK;
  const DaMask mk{mask, mask_stride_batch, mask_stride_head, mask_stride_query};
  hipStream_t stream = (hipStream_t)hip_stream;
  if (precision == DSPH_PREC_FP32)
    return dense_attention_backward_masked_fp32(q, k, v, ld, out, stat, mk, dout, delta, dq, dk, dv, ld_grad, N, M, heads, depth, stream);
  int64_t nblk;
  unsigned grid;
  rc = dense_grid(who, N, M, heads, &nblk, &grid);
  if (rc != DSPH_OK) return rc;
  const float scale = (float)(1.0 / std::sqrt((double)depth));
#define DENSE_BWD(DD, PP)                                                                                                                        \
  hipLaunchKernelGGL((dense_attention_split_dq_kernel<DD, PP, true, DaMask>), dim3(grid), dim3(256), 0, stream, q, k, v, ld, out, stat, dout, delta, dq, \
                     ld_grad, M, (int)heads, nblk, scale, mk);                                                                                   \
  hipLaunchKernelGGL((dense_attention_split_dkv_kernel<DD, PP, true, DaMask>), dim3(grid), dim3(256), 0, stream, q, k, v, ld, stat, dout, delta, dk, dv, \
                     ld_grad, M, (int)heads, nblk, scale, mk)
  DENSE_SPLIT_DISPATCH(depth, precision, DENSE_BWD);
#undef DENSE_BWD
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

}  // extern "C"
