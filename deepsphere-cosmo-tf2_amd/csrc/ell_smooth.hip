// One pass of a wide-row ELL matrix over a map with few channels: Gaussian smoothing of HEALPix maps.
//     y[n,m,c] = sum_j vals[m,j] * x[n, cols[m,j], c]                    (channel c smoothed in this pass)
//     y[n,m,c] = x[n,m,c]                                               (channel c passed through)
// times mask[m, c | 0] when a mask is given.  Replaces one utils.split_sparse_dense_matmul call per channel and repetition of
// the reference's HealpySmoothing.call (healpy_layers.py:725-764) together with its transposes, unstack / stack and the mask
// multiply; the same kernel on the transposed table is the input gradient.
//
// The shape is the opposite of the Chebyshev step's (cheb_step.hip): 1 - 8 channels, rows of tens to hundreds of entries that all
// have the same length W.  The table (8 W bytes per pixel) outweighs the map (4 C bytes per pixel and batch entry), so:
//   * a group of G lanes owns one output row (G = 16: one DPP row, W <= 128; G = 64: one wave, above).  Lane l keeps the entries
//     j = l, l + G, ... of the row-major [M][W] table in registers, E = ceil(W / G) <= 8 of them, so the table loads are
//     coalesced and happen ONCE per pass: the channel loop (in vectors of 4, 2 or 1 floats) and the batch loop run inside the
//     group, on the registers.  Rows wider than 8 G entries are worked through in chunks of 8 G, each chunk adding to what the
//     chunk before it stored (same lane, same address: ordered), so the table is still read once.
//   * the gathers of one (n, channel vector) are E independent loads per lane; W of them are in flight per row instead of the
//     chain of W dependent ones a thread per row would walk.
//   * the group's partial sums are added in a fixed butterfly (quad_perm, row_half_mirror, row_mirror inside the DPP row; two
//     xor shuffles across the rows of a 64-lane group).  No atomics, one writer per element: results are bitwise reproducible.
//   * rows are dealt to workgroups through xcd_remap: neighbouring NEST rows gather each other's pixels from one XCD's L2.
// Every pixel and element offset is 64-bit (N M C passes 2^31 at real sizes).  A table entry outside [0, M) counts as an empty
// slot (weight 0, the row's own pixel is read), so no table can make the kernel read out of bounds.
#include "dsphere_mapops.h"

namespace dsph {

namespace {

// v + (v of the lane the DPP control names); every lane of the wave is active where this is called
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}

// Sum over the G lanes of a group, the same bits in every lane: lanes 1 apart, 2 apart (quad_perm), the two quads of a half row
// (row_half_mirror: both hold their quad's sum, and a + b = b + a bit for bit), the two halves (row_mirror); G = 64: rows 16 and 32
// lanes apart.
template <int G>
__device__ __forceinline__ float group_sum(float v) {
  v = dpp_add<0xB1>(v);   // quad_perm [1, 0, 3, 2]
  v = dpp_add<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  v = dpp_add<0x141>(v);  // row_half_mirror
  v = dpp_add<0x140>(v);  // row_mirror
  if (G == 64) {
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
  }
  return v;
}

// G lanes per row, E table entries per lane and chunk, VEC channels per load
template <int G, int E, int VEC>
__global__ __launch_bounds__(256) void ell_smooth_kernel(const int32_t* __restrict__ cols, const float* __restrict__ vals, int64_t M,
                                                         int W, const float* __restrict__ x, float* __restrict__ y, int N, int C,
                                                         const int32_t* __restrict__ reps, int pass, const float* __restrict__ mask,
                                                         int mask_C, unsigned nblk) {
  constexpr int RPB = 256 / G;  // rows per workgroup
  const int64_t row = (int64_t)xcd_remap(blockIdx.x, nblk) * RPB + (int)(threadIdx.x / G);
  const int l = (int)(threadIdx.x % G);
  const bool valid = row < M;             // (the groups past the last row compute row M - 1 again and store nothing)
  const int64_t m = valid ? row : M - 1;
  const int nv = C / VEC;
  const int64_t plane = M * (int64_t)C;
  const int32_t* __restrict__ crow = cols + m * W;
  const float* __restrict__ vrow = vals + m * W;
  for (int j0 = 0; j0 < W; j0 += G * E) {
    const bool first = j0 == 0, last = j0 + G * E >= W;
    float kv[E];
    int64_t off[E];  // element offset of the entry's pixel inside one map
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int j = j0 + e * G + l;
      const int32_t c = j < W ? crow[j] : -1;
      const float k = j < W ? vrow[j] : 0.f;
      const bool ok = c >= 0 && (int64_t)c < M;
      kv[e] = ok ? k : 0.f;
      off[e] = (ok ? (int64_t)c : m) * C;
    }
    for (int q = 0; q < nv; ++q) {
      // the channels of this vector that this pass smooths (wave-uniform)
      unsigned act = 0;
#pragma unroll
      for (int u = 0; u < VEC; ++u) act |= (reps == nullptr || reps[q * VEC + u] > pass) ? (1u << u) : 0u;
      for (int n = 0; n < N; ++n) {
        const float* __restrict__ xn = x + n * plane + q * VEC;
        float acc[VEC];
#pragma unroll
        for (int u = 0; u < VEC; ++u) acc[u] = 0.f;
        if (act != 0) {
          float xv[E][VEC];
#pragma unroll
          for (int e = 0; e < E; ++e) ldv(xn + off[e], xv[e]);
#pragma unroll
          for (int e = 0; e < E; ++e)
#pragma unroll
            for (int u = 0; u < VEC; ++u) acc[u] = fmaf(kv[e], xv[e][u], acc[u]);
#pragma unroll
          for (int u = 0; u < VEC; ++u) acc[u] = group_sum<G>(acc[u]);
        }
        if (l == 0 && valid) {
          const int64_t o = n * plane + m * C + q * VEC;
          float r[VEC];
          if (!first && act != 0) {  // the chunks before this one
            ldv(y + o, r);
#pragma unroll
            for (int u = 0; u < VEC; ++u) r[u] += acc[u];
          } else {
#pragma unroll
            for (int u = 0; u < VEC; ++u) r[u] = acc[u];
          }
          if (act != (1u << VEC) - 1u) {  // channels passed through
            float own[VEC];
            ldv(x + o, own);
#pragma unroll
            for (int u = 0; u < VEC; ++u) r[u] = (act >> u & 1u) ? r[u] : own[u];
          }
          if (last && mask != nullptr) {
#pragma unroll
            for (int u = 0; u < VEC; ++u) r[u] *= mask[m * mask_C + (mask_C == 1 ? 0 : q * VEC + u)];
          }
          stv(y + o, r);
        }
      }
    }
  }
}

}  // namespace

}  // namespace dsph

extern "C" {

// one smoothing pass: every argument is checked here, before any launch
int dsph_ell_smooth(const int32_t* cols, const float* vals, int64_t M, int32_t W, const float* x, float* y, int64_t N, int32_t C,
                    const int32_t* reps, int32_t pass, const float* mask, int32_t mask_C, int device, void* hip_stream) {
  using namespace dsph;
  if (!cols || !vals || !x || !y) { set_error("ell_smooth: NULL pointer (cols, vals, x and y are required)"); return DSPH_E_BADARG; }
  if (N < 0 || M < 0) { set_error("ell_smooth: negative size (N %lld, M %lld)", (long long)N, (long long)M); return DSPH_E_BADARG; }
  if (M > 0x7fffffffLL) { set_error("ell_smooth: M = %lld exceeds the int32 column indices of the table", (long long)M); return DSPH_E_BADARG; }
  if (W <= 0) { set_error("ell_smooth: table width W = %d, must be at least 1", (int)W); return DSPH_E_BADARG; }
  if (C <= 0) { set_error("ell_smooth: C = %d channels, must be at least 1", (int)C); return DSPH_E_BADARG; }
  if (pass < 0) { set_error("ell_smooth: pass %d is negative", (int)pass); return DSPH_E_BADARG; }
  if (mask && mask_C != 1 && mask_C != C) {
    set_error("ell_smooth: mask_C = %d, the mask has 1 or C = %d columns", (int)mask_C, (int)C);
    return DSPH_E_BADARG;
  }
  const double elems = (double)N * (double)M * (double)C;
  if (elems >= 9.0e18 / 4) { set_error("ell_smooth: N * M * C = %.3g elements do not fit 64-bit byte offsets", elems); return DSPH_E_UNSUPPORTED; }
  const size_t bytes = (size_t)(N * M * (int64_t)C) * sizeof(float);
  if (ranges_overlap(x, bytes, y, bytes)) {  // (maps of no bytes overlap nothing)
    set_error("ell_smooth: x and y overlap; a pass reads neighbours of every row and cannot run in place");
    return DSPH_E_BADARG;
  }
  DeviceGuard guard(device);
  if (N <= 0 || M <= 0) return DSPH_OK;
  hipStream_t stream = (hipStream_t)hip_stream;
  const int G = W <= 128 ? 16 : 64;  // lanes that share one row of a table of width W
  const int E = (W + G - 1) / G < 8 ? (W + G - 1) / G : 8;
  const int VEC = vec_width(C, ptr_bits({x, y}), true);
  const int64_t nblk64 = (M + 256 / G - 1) / (256 / G);
  if (nblk64 > 0x7fffffffLL) { set_error("ell_smooth: grid too large (%lld workgroups)", (long long)nblk64); return DSPH_E_UNSUPPORTED; }
  const unsigned nblk = (unsigned)nblk64;
#define ELL_LAUNCH(GG, EE, VV)                                                                                                    \
  hipLaunchKernelGGL((ell_smooth_kernel<GG, EE, VV>), dim3(nblk), dim3(256), 0, stream, cols, vals, M, (int)W, x, y, (int)N, (int)C, \
                     reps, (int)pass, mask, (int)mask_C, nblk)
#define ELL_BY_VEC(GG, EE)                 \
  switch (VEC) {                           \
    case 4: ELL_LAUNCH(GG, EE, 4); break;  \
    case 2: ELL_LAUNCH(GG, EE, 2); break;  \
    default: ELL_LAUNCH(GG, EE, 1); break; \
  }
#define ELL_BY_E(GG)                   \
  switch (E) {                         \
    case 1: ELL_BY_VEC(GG, 1); break;  \
    case 2: ELL_BY_VEC(GG, 2); break;  \
    case 3: ELL_BY_VEC(GG, 3); break;  \
    case 4: ELL_BY_VEC(GG, 4); break;  \
    case 5: ELL_BY_VEC(GG, 5); break;  \
    case 6: ELL_BY_VEC(GG, 6); break;  \
    case 7: ELL_BY_VEC(GG, 7); break;  \
    default: ELL_BY_VEC(GG, 8); break; \
  }
  if (G == 16) {
    ELL_BY_E(16)
  } else {
    ELL_BY_E(64)
  }
#undef ELL_BY_E
#undef ELL_BY_VEC
#undef ELL_LAUNCH
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

}  // extern "C"
