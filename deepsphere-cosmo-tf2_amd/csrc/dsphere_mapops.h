// What the map operators share: the kernel families on channels-last (rows, channels) fp32 maps outside the Chebyshev plan
// (healpix_pool, nbr_attention, dense_attention, ell_smooth, basis_change, batch_norm, layer_norm, patch_gemm .hip).  Vector access
// and the merge of float64 partials on the device; the vector-width rule, the argument checks and the launch by width on the host.
// Only what two operators use.
#pragma once

#include <initializer_list>

#include "dsphere_common.h"

namespace dsph {

// VEC neighbouring floats in one access (VEC = 1, 2, 4; p aligned to 4 VEC bytes).  ldv<VEC>(p, r) and ldv(p, r) both resolve here.
template <int VEC>
__device__ __forceinline__ void ldv(const float* p, float (&r)[VEC]) {
  static_assert(VEC == 1 || VEC == 2 || VEC == 4, "ldv: 1, 2 or 4 floats");
  if constexpr (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w;
  } else if constexpr (VEC == 2) {
    const float2 t = *reinterpret_cast<const float2*>(p);
    r[0] = t.x; r[1] = t.y;
  } else {
    r[0] = *p;
  }
}
template <int VEC>
__device__ __forceinline__ void stv(float* p, const float (&r)[VEC]) {
  static_assert(VEC == 1 || VEC == 2 || VEC == 4, "stv: 1, 2 or 4 floats");
  if constexpr (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(r[0], r[1], r[2], r[3]);
  else if constexpr (VEC == 2) *reinterpret_cast<float2*>(p) = make_float2(r[0], r[1]);
  else *p = r[0];
}

inline uintptr_t ptr_bits(std::initializer_list<const void*> ps) {
  uintptr_t a = 0;
  for (const void* p : ps) a |= reinterpret_cast<uintptr_t>(p);
  return a;
}
inline bool aligned16(std::initializer_list<const void*> ps) { return (ptr_bits(ps) & 15) == 0; }

// Floats per access of a call: 4 where the channel count is a multiple of four and every map pointer (or-ed into `bits`; NULL adds
// nothing) is 16-byte aligned, 2 likewise (operators with a two-wide kernel: allow2), else 1
inline int vec_width(int channels, uintptr_t bits, bool allow2) {
  if (channels % 4 == 0 && (bits & 15) == 0) return 4;
  if (allow2 && channels % 2 == 0 && (bits & 7) == 0) return 2;
  return 1;
}

// do [p, p + bytes_p) and [q, q + bytes_q) meet (two empty ranges never do: a < b and b < a at once; NULL is an address like any
// other, so a caller with optional maps asks for non-NULL first)
inline bool ranges_overlap(const void* p, size_t bytes_p, const void* q, size_t bytes_q) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + bytes_q && b < a + bytes_p;
}

// the caller's scratch: large enough and aligned for float64 (a NULL one is named by the caller, among its required pointers)
inline bool workspace_ok(const char* who, const void* ptr, size_t have, size_t need, int* rc) {
  if (have < need) {
    set_error("%s: workspace of %zu bytes, %zu needed", who, have, need);
    *rc = DSPH_E_WORKSPACE;
    return false;
  }
  if (reinterpret_cast<uintptr_t>(ptr) & 7) {
    set_error("%s: workspace is not 8-byte aligned", who);
    *rc = DSPH_E_BADARG;
    return false;
  }
  return true;
}

// The second launch of a two-launch column reduction (layer_norm's dbeta / dgamma, patch_gemm's dbias): out[c] = the sum over p < NP of
// part[p * stride + blockIdx.y * ystep + c], c < n, in a fixed order -- a workgroup of MERGE_THREADS merges MERGE_COLS columns,
// MERGE_SLICES threads per column taking every MERGE_SLICES-th partial, then the first of them adds the others' sums in ascending
// order.  grid merge_grid(n, NOUT), NOUT = 1 or 2 outputs: row y of the grid writes out0 / out1 (a NULL one: nothing to do).
// (A template, so that only the operators that launch it carry it.)
constexpr int MERGE_THREADS = 256, MERGE_COLS = 16, MERGE_SLICES = MERGE_THREADS / MERGE_COLS;
template <int NOUT>
__global__ __launch_bounds__(MERGE_THREADS) void partials_merge_kernel(const double* __restrict__ part, int64_t NP, int64_t stride, int64_t ystep,
                                                                             int32_t n, float* __restrict__ out0, float* __restrict__ out1) {
  __shared__ double acc[MERGE_SLICES][MERGE_COLS];
  float* out = (NOUT > 1 && blockIdx.y) ? out1 : out0;
  if (!out) return;  // (the whole workgroup)
  part += (int64_t)blockIdx.y * ystep;
  const int cl = (int)threadIdx.x % MERGE_COLS, s = (int)threadIdx.x / MERGE_COLS;
  const int c = (int)blockIdx.x * MERGE_COLS + cl;
  double v = 0.0;
  if (c < n)
    for (int64_t p = s; p < NP; p += MERGE_SLICES) v += part[p * stride + c];
  acc[s][cl] = v;
  __syncthreads();
  if (s == 0 && c < n) {
    for (int t = 1; t < MERGE_SLICES; ++t) v += acc[t][cl];
    out[c] = (float)v;
  }
}
inline dim3 merge_grid(int32_t n, int outputs) { return dim3((unsigned)((n + MERGE_COLS - 1) / MERGE_COLS), (unsigned)outputs); }

inline bool select_device(const char* who, int device, const DeviceGuard& guard) {
  if (!guard.ok) set_error("%s: cannot select device %d", who, device);
  return guard.ok;
}

// The limits both attention families put on a row: one of five depths per head and at most 256 channels (`why`: what the message
// adds to that rule, "" for nothing), then rows a multiple of four floats apart.  Two steps: the neighbour table's own rule sits
// between them.
inline int attention_shape_ok(const char* who, int32_t heads, int32_t depth, const char* why) {
  if (depth != 4 && depth != 8 && depth != 16 && depth != 32 && depth != 64) {
    set_error("%s: depth %d per head is not one of 4, 8, 16, 32, 64", who, (int)depth);
    return DSPH_E_BADARG;
  }
  if (heads < 1 || (int64_t)heads * depth > 256) {
    set_error("%s: heads * depth = %d * %d must lie in [depth, 256]%s", who, (int)heads, (int)depth, why);
    return DSPH_E_BADARG;
  }
  return DSPH_OK;
}
inline int attention_stride_ok(const char* who, int64_t ld, int32_t heads, int32_t depth) {
  if (ld % 4 != 0 || ld < (int64_t)heads * depth) {
    set_error("%s: row stride %lld must be a multiple of 4 floats and at least heads * depth = %d", who, (long long)ld, (int)(heads * depth));
    return DSPH_E_BADARG;
  }
  return DSPH_OK;
}

}  // namespace dsph

// KERNEL<4>, <2> or <1> by the call's vec_width
#define DSPH_LAUNCH_BY_VEC(vec, KERNEL, grid, block, stream, ...)                                   \
  switch (vec) {                                                                                    \
    case 4: hipLaunchKernelGGL((KERNEL<4>), grid, block, 0, stream, __VA_ARGS__); break;            \
    case 2: hipLaunchKernelGGL((KERNEL<2>), grid, block, 0, stream, __VA_ARGS__); break;            \
    default: hipLaunchKernelGGL((KERNEL<1>), grid, block, 0, stream, __VA_ARGS__); break;           \
  }
