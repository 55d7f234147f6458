// Dense attention on the bf16 matrix pipe: the arithmetic policy that runs the kernels of dense_attention_kernel.h (same blocking,
// same contract, same outputs as fp32) with every product on v_mfma_f32_16x16x32_bf16 through a split of its fp32 operands, fp32
// accumulation:
//   DSPH_PREC_BF16X3   a = hi + lo         products hh + hl + lh                     (2^-16 relative per operand)
//   DSPH_PREC_BF16X6   a = hi + mid + lo   products hh + hm + mh + hl + lh + mm      (fp32-equivalent)
// Each term is the round-to-nearest bf16 of the running remainder (a - hi and a - hi - mid are exact in fp32); bf16 has fp32's
// exponent range, so there is no scale rule.  The softmax statistics, exp, lse, delta and every rescaling stay fp32 on the vector
// unit; the mask's addend goes onto the fp32 logit after the product (it is never split).
// Depths 32 and 64: the contraction of the first product is one or two full K = 32 steps.
//
// Tiles are TS rows (64; 32 where the images of a 64-row tile pass 64 KiB: the six-term backward and the three-term dk / dv at
// depth 64).  A tile is split ONCE, at staging, into bf16 planes per term, in up to two images:
//   row image  [term][TS][D]       the A operand of the first product  S^T = T O^T  (T the tile, O the owned rows, split once into
//                                  registers as the B operand): lane l reads channels 32 ks + 8 (l / 16) + j, j = 0..7, of tile
//                                  row 16 sub + l % 16 -- 16 bytes, conflict-free under the chunk swizzle of off().
//   transposed [term][D][TS]       the A operand of the second product  acc^T += T'^T X^T  (X = P or dS), which sums over tile
//                                  rows.  The first product leaves lane l with S(tile row 16 sub + 4 g + r, owned row l % 16),
//                                  g = l / 16, in register r of sub-tile sub; the B operand of 16x16x32 wants k = 8 g + j, j = 0..7,
//                                  for column l % 16.  So step u of the second product takes the sub-tiles 2 u and 2 u + 1: its
//                                  element j is register j % 4 of sub-tile 2 u + j / 4, i.e. k = 8 g + j is tile row
//                                  16 (2 u + j / 4) + 4 g + j % 4, and the softmax feeds the MFMA from registers, no LDS.  The
//                                  image stores tile row t at position 32 u + 8 g + 4 (j / 4) + j % 4 of its channel (das_pos),
//                                  which makes the A operand -- channel 16 b + l % 16, those eight rows -- 16 contiguous bytes.
// P and dS are split per element in registers.
#include "dense_attention_kernel.h"

namespace dsph {

typedef __bf16 das_bf16x8 __attribute__((ext_vector_type(8)));

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
__device__ __forceinline__ da_f32x4 das_mfma(const DasFrag<NT>& a, const DasFrag<NT>& b, da_f32x4 c) {
  if constexpr (NT == 3) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.t[0], b.t[2], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.t[2], b.t[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.t[1], b.t[1], c, 0, 0, 0);
  }
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.t[0], b.t[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.t[1], b.t[0], c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.t[0], b.t[0], c, 0, 0, 0);
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

// position of tile row t in a channel of the transposed image
__device__ __forceinline__ int das_pos(int t) { return (t & ~31) | ((t & 12) << 1) | ((t & 16) >> 2) | (t & 3); }

// NT terms per operand; KIND the kernel (0 forward, 1 dq, 2 dk / dv), which sets the tile rows
template <int DEPTH, int NT, int KIND>
struct DaSplit {
  static constexpr int D = DEPTH;
  static constexpr int TS = das_tile_rows(KIND, D, NT);
  static_assert((D == 32 || D == 64) && (TS == 32 || TS == 64), "depths 32 and 64, tiles of 32 or 64 rows");
  static_assert(KIND != 2 || das_lds_bytes(2, D, TS, NT) + TS * 4 <= 64 * 1024,
                "the second statistic of a masked dk / dv keeps the tile rows das_tile_rows chose");
  static constexpr int KS = D / 32;             // K = 32 steps of the first product
  static constexpr int CB = D / 16;             // 16-channel blocks of the accumulator
  static constexpr int NSUB = TS / 16;          // 16-row sub-tiles of a tile
  static constexpr int NU = TS / 32;            // K = 32 steps of the second product
  static constexpr int ROWIMG = TS * D;         // bf16 of one term's plane, row image [TS][D] and transposed image [D][TS]
  static constexpr int TRIMG = D * TS;
  static constexpr int RPT = TS * (D / 4) / 256;  // staging: a thread holds 4 channels of RPT neighbouring rows
  static_assert(RPT == 2 || RPT == 4, "a thread packs 2 or 4 rows of a channel into one transposed store");

  struct Own {
    DasFrag<NT> f[KS];
    float raw[KS][8];  // the fp32 channels (dq: for delta)
  };
  typedef float4 Stage[RPT];
  // the images IMG of a tile, the row image first
  template <int IMG>
  struct __attribute__((aligned(16))) Tile {
    static constexpr int TR_AT = IMG & DA_ROW ? NT * ROWIMG : 0;  // where the transposed image starts
    __bf16 e[TR_AT + (IMG & DA_TR ? NT * TRIMG : 0)];
  };

  // the owned row's B operand of the first product: step ks holds channels 32 ks + 8 g + j; zeros for a row past M
  static __device__ __forceinline__ void load_own(Own& o, const float* row, bool, int g) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
      if (row != nullptr) {
        lo = *reinterpret_cast<const float4*>(row + 32 * ks + 8 * g);
        hi = *reinterpret_cast<const float4*>(row + 32 * ks + 8 * g + 4);
      }
      o.raw[ks][0] = lo.x; o.raw[ks][1] = lo.y; o.raw[ks][2] = lo.z; o.raw[ks][3] = lo.w;
      o.raw[ks][4] = hi.x; o.raw[ks][5] = hi.y; o.raw[ks][6] = hi.z; o.raw[ks][7] = hi.w;
      o.f[ks] = das_split8<NT>(o.raw[ks]);
    }
  }

  // the lane group's part of dout . out of an owned row, gf its dout
  static __device__ __forceinline__ float out_dot(const Own& gf, const float* orow, int g) {
    float dl = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int j = 0; j < 8; ++j) dl = fmaf(gf.raw[ks][j], orow[32 * ks + 8 * g + j], dl);
    return dl;
  }

  // c[r] = (row 16 sub + 4 g + r of the tile) . (the owned row of lane % 16), from the tile's row image
  template <int IMG>
  static __device__ __forceinline__ da_f32x4 tile_dot(const Tile<IMG>& tile, int sub, const Own& own, int lane) {
    static_assert(IMG & DA_ROW, "a tile staged for the first product");
    da_f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const __bf16* p = tile.e + das_off<D>(16 * sub + (lane & 15), 32 * ks + 8 * (lane >> 4));
      DasFrag<NT> a;
#pragma unroll
      for (int i = 0; i < NT; ++i) a.t[i] = *reinterpret_cast<const das_bf16x8*>(p + i * ROWIMG);
      c = das_mfma<NT>(a, own.f[ks], c);
    }
    return c;
  }

  // The second product, issued once per tile: acc[b][r'] (channel 16 b + 4 g + r', owned row lane % 16) += sum over the tile rows t
  // of tile[t][channel] x(t), x[sub][r] being what tile_dot returned for sub-tile sub, after the softmax; from the transposed image
  struct Sink {
    da_f32x4 x[NSUB];
    template <int IMG>
    __device__ __forceinline__ void push(da_f32x4 (&)[CB], const Tile<IMG>&, int sub, const da_f32x4& xs, int) { x[sub] = xs; }
    template <int IMG>
    __device__ __forceinline__ void flush(da_f32x4 (&acc)[CB], const Tile<IMG>& tile, int lane) {
      static_assert(IMG & DA_TR, "a tile staged for the second product");
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        const float xv[8] = {x[2 * u][0], x[2 * u][1], x[2 * u][2], x[2 * u][3], x[2 * u + 1][0], x[2 * u + 1][1], x[2 * u + 1][2], x[2 * u + 1][3]};
        const DasFrag<NT> xb = das_split8<NT>(xv);
#pragma unroll
        for (int b = 0; b < CB; ++b) {
          const __bf16* p = tile.e + Tile<IMG>::TR_AT + das_off<TS>(16 * b + (lane & 15), 32 * u + 8 * (lane >> 4));
          DasFrag<NT> a;
#pragma unroll
          for (int i = 0; i < NT; ++i) a.t[i] = *reinterpret_cast<const das_bf16x8*>(p + i * TRIMG);
          acc[b] = das_mfma<NT>(a, xb, acc[b]);
        }
      }
    }
  };

  // staging: thread tid holds channels [4 c4, 4 c4 + 4) of the rows RPT a + i, c4 = tid % (D / 4), a = tid / (D / 4).
  // global -> registers (zeros past `valid`)
  static __device__ __forceinline__ void stage_load(Stage& s, const float* __restrict__ src, int64_t ld, int valid, int tid) {
    const int c4 = tid % (D / 4), r0 = tid / (D / 4) * RPT;
#pragma unroll
    for (int i = 0; i < RPT; ++i)
      s[i] = r0 + i < valid ? *reinterpret_cast<const float4*>(src + (r0 + i) * ld + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
  }

  // registers -> the split planes of the tile's images
  template <int IMG>
  static __device__ __forceinline__ void stage_store(const Stage& s, Tile<IMG>* tile, int tid) {
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
    __bf16* rimg = IMG & DA_ROW ? tile->e : nullptr;  // (nullptr: the kernel has no such image)
    __bf16* timg = IMG & DA_TR ? tile->e + Tile<IMG>::TR_AT : nullptr;
    if (rimg != nullptr) {
#pragma unroll
      for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int i = 0; i < RPT; ++i)
          *reinterpret_cast<bf16x4*>(rimg + n * ROWIMG + das_off<D>(r0 + i, 4 * c4)) = bf16x4{t[i][0][n], t[i][1][n], t[i][2][n], t[i][3][n]};
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
          *reinterpret_cast<bf16xr*>(timg + n * TRIMG + das_off<TS>(4 * c4 + c, pos)) = v;
        }
    }
  }

  // the lane's accumulator, times f, to channels [16 b + 4 g, + 4) of its row
  static __device__ __forceinline__ void store_acc(float* rowp, const da_f32x4 (&acc)[CB], float f, int g) {
#pragma unroll
    for (int b = 0; b < CB; ++b)
      *reinterpret_cast<float4*>(rowp + 16 * b + 4 * g) = make_float4(acc[b][0] * f, acc[b][1] * f, acc[b][2] * f, acc[b][3] * f);
  }
};

// the split launches: the policy from the depth (32 or 64) and the precision (one of the two splits), both checked by the caller
template <int DEPTH, int NT>
static void dense_split_launch(const DenseCall& c, bool backward) {
  if (backward) dense_launch_backward<DaSplit<DEPTH, NT, 1>, DaSplit<DEPTH, NT, 2>>(c); else dense_launch_forward<DaSplit<DEPTH, NT, 0>>(c);
}
static void dense_split_launch(const DenseCall& c, bool backward) {
  if (c.precision == DSPH_PREC_BF16X6) {
    if (c.depth == 32) dense_split_launch<32, 3>(c, backward); else dense_split_launch<64, 3>(c, backward);
  } else {
    if (c.depth == 32) dense_split_launch<32, 2>(c, backward); else dense_split_launch<64, 2>(c, backward);
  }
}
void dense_split_launch_forward(const DenseCall& c) { dense_split_launch(c, false); }
void dense_split_launch_backward(const DenseCall& c) { dense_split_launch(c, true); }

}  // namespace dsph
