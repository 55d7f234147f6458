// Dense attention: the exact-fp32 arithmetic of the kernels in dense_attention_kernel.h, and the entry points of every arithmetic.
//
// All products run on the exact-fp32 MFMA v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain, no reduced precision, no range
// condition), depths 4 to 64.  Tiles are 64 rows.  Step r of the second product sums over the tile rows 4 g + r, g = 0..3, which
// is the register order in which the first product left them, so the softmax feeds it from registers.
//
// LDS tiles are [64][D + 4] floats (D = 4: [64][4]): rows 16 bytes aligned, and both read patterns (16 rows x 4 channel groups
// for the first product, 4 rows x 16 channels for the second) fall on 64 different banks; one tile serves both products.
#include <cmath>
#include <string>

#include "dense_attention_kernel.h"

namespace dsph {

template <int DEPTH>
struct DaFp32 {
  static constexpr int D = DEPTH;
  static constexpr int TS = DA_TILE;                              // rows of a streamed tile
  static constexpr int NSUB = TS / 16;
  static constexpr int STRIDE = D == 4 ? 4 : D + 4;               // floats between the rows of an LDS tile
  static constexpr int NF = D / 4;                                // registers of a lane's row fragment = MFMA steps of a dot product
  static constexpr int CB = (D + 15) / 16;                        // 16-channel blocks of the accumulator
  static constexpr int STAGE = (TS * (D / 4) + 255) / 256;        // 16-byte pieces of a tile per thread

  typedef float Own[NF];  // a row's fragment, below
  typedef float4 Stage[STAGE];
  template <int IMG>
  struct __attribute__((aligned(16))) Tile {
    float e[TS * STRIDE];
  };

  // A lane's fragment of one row: the channels that its lane group g = lane / 16 contributes to the dot product, fragment element e
  // being MFMA step e (both operands use this one map, so any map is right; this one makes the loads 16 bytes wide).
  // D >= 16: element 4 b + s is channel 16 b + 4 g + s;  D = 8: element s is channel 2 g + s;  D = 4: channel g.
  static __device__ __forceinline__ void load_frag(Own& o, const float* row, int g) {
    if constexpr (D >= 16) {
#pragma unroll
      for (int b = 0; b < D / 16; ++b) {
        const float4 t = *reinterpret_cast<const float4*>(row + 16 * b + 4 * g);
        o[4 * b] = t.x; o[4 * b + 1] = t.y; o[4 * b + 2] = t.z; o[4 * b + 3] = t.w;
      }
    } else if constexpr (D == 8) {
      const float2 t = *reinterpret_cast<const float2*>(row + 2 * g);
      o[0] = t.x; o[1] = t.y;
    } else {
      o[0] = row[g];
    }
  }

  // the owned row's B operand of the first product; zeros for a row past M
  static __device__ __forceinline__ void load_own(Own& o, const float* row, bool own, int g) {
    if (own) {
      load_frag(o, row, g);
    } else {
#pragma unroll
      for (int e = 0; e < NF; ++e) o[e] = 0.f;
    }
  }

  // the lane group's part of dout . out of an owned row, gf its dout fragment
  static __device__ __forceinline__ float out_dot(const Own& gf, const float* orow, int g) {
    Own of;
    load_frag(of, orow, g);
    float dl = 0.f;
#pragma unroll
    for (int e = 0; e < NF; ++e) dl = fmaf(gf[e], of[e], dl);
    return dl;
  }

  // c[r] = (row 16 sub + 4 g + r of the LDS tile) . (the owned row of lane % 16, fragment `own`)
  template <int IMG>
  static __device__ __forceinline__ da_f32x4 tile_dot(const Tile<IMG>& tile, int sub, const Own& own, int lane) {
    static_assert(IMG & DA_ROW, "a tile staged for the first product");
    Own a;
    load_frag(a, tile.e + (16 * sub + (lane & 15)) * STRIDE, lane >> 4);
    da_f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < NF; ++e) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], own[e], c, 0, 0, 0);
    return c;
  }

  // The second product, issued per sub-tile: acc[b][r'] (channel 16 b + 4 g + r', owned row lane % 16) += sum over the tile rows
  // t = 16 sub + 4 g' + r of tile[t][channel] x(t), x(t) being register r of the lanes of group g': what tile_dot returned, after the
  // softmax
  struct Sink {
    template <int IMG>
    __device__ __forceinline__ void push(da_f32x4 (&acc)[CB], const Tile<IMG>& tile, int sub, const da_f32x4& x, int lane) {
      static_assert(IMG & DA_TR, "a tile staged for the second product");
      const int g = lane >> 4, c = lane & 15;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* row = tile.e + (16 * sub + 4 * g + r) * STRIDE;
#pragma unroll
        for (int b = 0; b < CB; ++b) {
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
    template <int IMG>
    __device__ __forceinline__ void flush(da_f32x4 (&)[CB], const Tile<IMG>&, int) {}
  };

  // a tile of `valid` (<= 64) rows, D channels from src on, rows ld apart: global -> registers, registers -> LDS (zeros past `valid`)
  static __device__ __forceinline__ void stage_load(Stage& s, const float* __restrict__ src, int64_t ld, int valid, int tid) {
#pragma unroll
    for (int i = 0; i < STAGE; ++i) {
      const int idx = tid + 256 * i, row = idx / (D / 4), c4 = idx % (D / 4);
      s[i] = row < valid ? *reinterpret_cast<const float4*>(src + row * ld + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }

  template <int IMG>
  static __device__ __forceinline__ void stage_store(const Stage& s, Tile<IMG>* tile, int tid) {
#pragma unroll
    for (int i = 0; i < STAGE; ++i) {
      const int idx = tid + 256 * i, row = idx / (D / 4), c4 = idx % (D / 4);
      if (row < TS) *reinterpret_cast<float4*>(tile->e + row * STRIDE + 4 * c4) = s[i];
    }
  }

  // the lane's accumulator, times f, to channels [16 b + 4 g, + 4) of its row
  static __device__ __forceinline__ void store_acc(float* rowp, const da_f32x4 (&acc)[CB], float f, int g) {
#pragma unroll
    for (int b = 0; b < CB; ++b)
      if (16 * b + 4 * g < D) *reinterpret_cast<float4*>(rowp + 16 * b + 4 * g) = make_float4(acc[b][0] * f, acc[b][1] * f, acc[b][2] * f, acc[b][3] * f);
  }
};

// the fp32 launches: the policy from the depth (checked: 4, 8, 16, 32 or 64)
template <int DEPTH>
static void dense_fp32_launch(const DenseCall& c, bool backward) {
  if (backward) dense_launch_backward<DaFp32<DEPTH>, DaFp32<DEPTH>>(c); else dense_launch_forward<DaFp32<DEPTH>>(c);
}
static void dense_fp32_launch(const DenseCall& c, bool backward) {
  switch (c.depth) {
    case 4: dense_fp32_launch<4>(c, backward); break;
    case 8: dense_fp32_launch<8>(c, backward); break;
    case 16: dense_fp32_launch<16>(c, backward); break;
    case 32: dense_fp32_launch<32>(c, backward); break;
    default: dense_fp32_launch<64>(c, backward); break;
  }
}

// the precision code of a call: DSPH_PREC_FP32 and the two splits; a split runs depths 32 and 64 only
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

// Every entry point: the checks, in one order (pointers, mask, shapes, precision, alignment), then the launch.  `who` names the
// call in its messages; `masked` calls carry a mask operand and the pair statistic, which they want 8-byte aligned; `backward`
// calls carry the gradient fields of `c`.
static int dense_attention_call(const char* who, bool masked, bool backward, DenseCall c, int device, void* hip_stream) {
  bool null = !c.q || !c.k || !c.v || !c.out;
  if (backward) null = null || !c.stat || !c.dout || !c.delta || !c.dq || !c.dk || !c.dv;
  if (null) { set_error("%s: NULL pointer", who); return DSPH_E_BADARG; }
  int rc = masked ? dense_mask_args_ok(who, c.mk.p, c.mk.sb, c.mk.sh, c.mk.sq) : DSPH_OK;
  if (rc == DSPH_OK) rc = dense_attention_args_ok(who, c.ld, c.N, c.M, c.heads, c.depth);
  if (rc == DSPH_OK && backward) rc = dense_attention_args_ok((std::string(who) + " (gradients)").c_str(), c.ld_grad, c.N, c.M, c.heads, c.depth);
  if (rc == DSPH_OK) rc = dense_precision_ok(who, c.precision, c.depth);
  if (rc != DSPH_OK) return rc;
  const bool aligned = backward ? aligned16({c.q, c.k, c.v, c.out, c.dout, c.dq, c.dk, c.dv}) : aligned16({c.q, c.k, c.v, c.out});
  if (!aligned || (masked && (reinterpret_cast<uintptr_t>(c.stat) & 7) != 0)) {
    set_error("%s: %s must be 16-byte aligned%s", who, backward ? "q, k, v, out, dout, dq, dk and dv" : "q, k, v and out", masked ? ", stat 8-byte" : "");
    return DSPH_E_BADARG;
  }
  DeviceGuard guard(device);
  if (c.N <= 0 || c.M <= 0) return DSPH_OK;
  rc = dense_grid(who, c.N, c.M, c.heads, &c.nblk, &c.grid);
  if (rc != DSPH_OK) return rc;
  c.scale = (float)(1.0 / std::sqrt((double)c.depth));
  c.stream = (hipStream_t)hip_stream;
  if (c.precision == DSPH_PREC_FP32) dense_fp32_launch(c, backward);
  else if (backward) dense_split_launch_backward(c);
  else dense_split_launch_forward(c);
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

}  // namespace dsph

extern "C" {

int dsph_dense_attention_forward_prec(const float* q, const float* k, const float* v, int64_t ld, float* out, float* lse, int64_t N,
                                      int64_t M, int32_t heads, int32_t depth, int32_t precision, int device, void* hip_stream) {
  dsph::DenseCall c = {q, k, v, ld, out, lse};
  c.N = N; c.M = M; c.heads = heads; c.depth = depth; c.precision = precision;
  return dsph::dense_attention_call("dense_attention_forward", false, false, c, device, hip_stream);
}

int dsph_dense_attention_backward_prec(const float* q, const float* k, const float* v, int64_t ld, const float* out, const float* lse,
                                       const float* dout, float* delta, float* dq, float* dk, float* dv, int64_t ld_grad, int64_t N,
                                       int64_t M, int32_t heads, int32_t depth, int32_t precision, int device, void* hip_stream) {
  dsph::DenseCall c = {q, k, v, ld, const_cast<float*>(out), const_cast<float*>(lse), {}, dout, delta, dq, dk, dv, ld_grad};
  c.N = N; c.M = M; c.heads = heads; c.depth = depth; c.precision = precision;
  return dsph::dense_attention_call("dense_attention_backward", false, true, c, device, hip_stream);
}

int dsph_dense_attention_forward(const float* q, const float* k, const float* v, int64_t ld, float* out, float* lse, int64_t N, int64_t M,
                                 int32_t heads, int32_t depth, int device, void* hip_stream) {
  return dsph_dense_attention_forward_prec(q, k, v, ld, out, lse, N, M, heads, depth, DSPH_PREC_FP32, device, hip_stream);
}

int dsph_dense_attention_backward(const float* q, const float* k, const float* v, int64_t ld, const float* out, const float* lse,
                                  const float* dout, float* delta, float* dq, float* dk, float* dv, int64_t ld_grad, int64_t N, int64_t M,
                                  int32_t heads, int32_t depth, int device, void* hip_stream) {
  return dsph_dense_attention_backward_prec(q, k, v, ld, out, lse, dout, delta, dq, dk, dv, ld_grad, N, M, heads, depth, DSPH_PREC_FP32, device,
                                            hip_stream);
}

int dsph_dense_attention_forward_masked(const float* q, const float* k, const float* v, int64_t ld, float* out, float* stat, const float* mask,
                                        int64_t mask_stride_batch, int64_t mask_stride_head, int64_t mask_stride_query, int64_t N, int64_t M,
                                        int32_t heads, int32_t depth, int32_t precision, int device, void* hip_stream) {
  dsph::DenseCall c = {q, k, v, ld, out, stat, {mask, mask_stride_batch, mask_stride_head, mask_stride_query}};
  c.N = N; c.M = M; c.heads = heads; c.depth = depth; c.precision = precision;
  return dsph::dense_attention_call("dense_attention_forward_masked", true, false, c, device, hip_stream);
}

int dsph_dense_attention_backward_masked(const float* q, const float* k, const float* v, int64_t ld, const float* out, const float* stat,
                                         const float* mask, int64_t mask_stride_batch, int64_t mask_stride_head, int64_t mask_stride_query,
                                         const float* dout, float* delta, float* dq, float* dk, float* dv, int64_t ld_grad, int64_t N, int64_t M,
                                         int32_t heads, int32_t depth, int32_t precision, int device, void* hip_stream) {
  dsph::DenseCall c = {q, k, v, ld, const_cast<float*>(out), const_cast<float*>(stat), {mask, mask_stride_batch, mask_stride_head, mask_stride_query},
                       dout, delta, dq, dk, dv, ld_grad};
  c.N = N; c.M = M; c.heads = heads; c.depth = depth; c.precision = precision;
  return dsph::dense_attention_call("dense_attention_backward_masked", true, true, c, device, hip_stream);
}

}  // extern "C"
