// Rotating HEALPix maps by bilinear interpolation (healpy's get_interpol / Rotator.rotate_map_pixel; healpy_layers.HealpyRotate here):
//   y[n, r, :] = sum_j w_j x[n, row(p_j), :],  (p_j, w_j) the four-pixel stencil at R^T v(indices[r]),  R = rot[n]
// pixel -> centre vector -> rotated direction -> the two rings that bracket its colatitude -> on either ring the two pixels that
// bracket its phi -> gather.  Nothing is materialised: a table of the same stencils (dsph_healpix_interp_table) is 32 bytes per
// pixel and rotation, 400 MB at nside 1024, and a training loop draws a fresh rotation per sample and step.
//
// The stencil (interp_stencil, host and device, float64 throughout): ring_above(z) and the ring below it; on a ring of n pixels with
// step dphi, tmp = phi / dphi - shift / 2, i1 = floor(tmp), w1 = (phi - (i1 + shift / 2) dphi) / dphi, pixels i1 and i1 + 1 BOTH
// wrapped modulo n (phi is reduced into [0, 2 pi], and a phi of -1e-17 reduces to exactly 2 pi, where i1 = n on an unshifted ring);
// the two rings mixed linearly in theta.  Above the first ring the ring's weights are scaled by theta / theta_1 and the rest,
// (1 - wtheta) / 4 a pixel, goes to all four pixels of ring 1 (partners two positions on); below the last ring likewise.  A row
// never holds a pixel twice: two positions of a ring differ (a ring has at least 4 pixels), the rings differ, and in the pole
// branches the four pixels are all of the polar ring.  wtheta is clamped to [0, 1]: at a ring's own latitude ring_above may
// name the ring above it, where wtheta is 1 up to rounding; the interpolant is continuous there.
//
// Weights are rounded to float32 once; y = w0 x0, then three fmaf in the order of the stencil: the same arithmetic in every form of
// the kernel, no atomics.  A source pixel outside a partial-sky set contributes an explicit 0 (the rotated zero-padded map).
//
// Output pixels are taken in blocks of HI_BLOCK consecutive rows -- an aligned NEST block of 16 x 16 pixels on the full sky -- and the
// blocks are dealt to the XCDs in contiguous ranges (xcd_remap): a rotated block is a compact patch of the source, about 17 rows of
// 17 pixels, and neighbouring blocks' patches overlap, so source rows are served from one L2.
// Two forms by F, as healpix_reorder.hip has:
//   narrow rows (F < HI_WIDE_F): a lane owns a pixel, its stencil in registers, its four gathers VEC floats at a time;
//   wide rows: the block's stencils go to LDS (4 x (int32 row, float32 weight) per pixel), then F / VEC consecutive lanes run along
//     a row, HI_BATCH items per lane in flight (4 HI_BATCH gathers).
// Grid: x = the blocks of a map (at most 12 * 8192^2 / 256 = 3,145,728), y = min(N, 65535) samples, further samples on further trips.
// With one rotation for the whole batch (n_rot = 1) a workgroup computes its stencils once and keeps them over its loop over
// samples, and y shrinks to what still fills the chip (1 from nside 256 up): the float64 geometry, which bounds the narrow forms
// (about 30 G stencils / s), is then paid once per pixel instead of once per sample and pixel.
#include <algorithm>
#include <cmath>

#include "dsphere_mapops.h"
#include "healpix_ring.h"

namespace dsph {

constexpr int HI_BLOCK = 256;        // output pixels of a workgroup = its threads
constexpr int HI_WIDE_F = 16;        // rows of 16 floats or more: lanes along the channels
constexpr int HI_BATCH = 2;          // items a lane of the wide form keeps in flight
constexpr int HI_MAX_NSIDE = 8192;   // 12 nside^2 - 1 fits int32 up to here
constexpr int HI_MAX_GRID_Y = 65535;
constexpr int HI_FILL_GROUPS = 4096; // workgroups that fill the chip (256 CUs x 4 resident) four times over

// the two pixels of ring g that bracket phi in [0, 2 pi] (positions 1 .. 4 nr) and the weight of the second
__host__ __device__ __forceinline__ void interp_ring_pair(const KnnRing& g, double phi, int32_t* j1, int32_t* j2, double* w1) {
  const int32_t n4 = 4 * g.nr;
  const double half = 0.5 * (double)knn_ring_shifted(g);
  const double fl = floor(phi / g.step - half);  // -1 .. n4
  *w1 = (phi - (fl + half) * g.step) / g.step;
  int32_t i1 = (int32_t)fl % n4;
  if (i1 < 0) i1 += n4;
  const int32_t i2 = i1 + 1 < n4 ? i1 + 1 : 0;
  *j1 = i1 + 1; *j2 = i2 + 1;
}

// The interpolation stencil at the direction (z = cos theta, theta, phi in [0, 2 pi]): four NEST ids and float64 weights
__host__ __device__ __forceinline__ void interp_stencil(int32_t nside, int32_t lgn, double z, double theta, double phi, int32_t (&pix)[4],
                                                        double (&w)[4]) {
  const int32_t nl4 = 4 * nside;
  const int32_t ir1 = knn_ring_above(nside, z), ir2 = ir1 + 1;
  const bool north = ir1 <= 0, south = ir2 >= nl4;  // beyond the first / the last ring: all four pixels from that ring
  const KnnRing g1 = knn_ring(nside, north ? 1 : ir1), g2 = knn_ring(nside, south ? nl4 - 1 : ir2);
  const double th1 = atan2(g1.st, g1.z), th2 = atan2(g2.st, g2.z);
  int32_t jp[4];
  double w1;
  interp_ring_pair(g1, phi, &jp[0], &jp[1], &w1);
  w[0] = 1.0 - w1; w[1] = w1;
  interp_ring_pair(g2, phi, &jp[2], &jp[3], &w1);
  w[2] = 1.0 - w1; w[3] = w1;
  if (north) {  // (g1 == g2 == ring 1: entries 2, 3 bracket phi, entries 0, 1 are their partners across the pole)
    const double wt = fmin(fmax(theta / th2, 0.0), 1.0), fac = (1.0 - wt) * 0.25;
    w[2] = w[2] * wt + fac; w[3] = w[3] * wt + fac;
    w[0] = fac; w[1] = fac;
    jp[0] = ((jp[2] + 1) & 3) + 1; jp[1] = ((jp[3] + 1) & 3) + 1;  // position (i + 2) & 3, one-based
  } else if (south) {
    const double wt = fmin(fmax((theta - th1) / (M_PI - th1), 0.0), 1.0), fac = wt * 0.25;
    w[0] = w[0] * (1.0 - wt) + fac; w[1] = w[1] * (1.0 - wt) + fac;
    w[2] = fac; w[3] = fac;
    jp[2] = ((jp[0] + 1) & 3) + 1; jp[3] = ((jp[1] + 1) & 3) + 1;
  } else {
    const double wt = fmin(fmax((theta - th1) / (th2 - th1), 0.0), 1.0);
    w[0] *= 1.0 - wt; w[1] *= 1.0 - wt;
    w[2] *= wt; w[3] *= wt;
  }
  const int32_t r1 = north ? 1 : ir1, r2 = south ? nl4 - 1 : ir2;
  pix[0] = knn_ring_to_nest(nside, lgn, r1, g1.nr, g1.kshift, jp[0]);
  pix[1] = knn_ring_to_nest(nside, lgn, r1, g1.nr, g1.kshift, jp[1]);
  pix[2] = knn_ring_to_nest(nside, lgn, r2, g2.nr, g2.kshift, jp[2]);
  pix[3] = knn_ring_to_nest(nside, lgn, r2, g2.nr, g2.kshift, jp[3]);
}

// The stencil of output pixel `pix` (NEST) under the rotation R (row-major 3 x 3): the source direction is R^T v(pix)
__host__ __device__ __forceinline__ void rotated_stencil(int32_t nside, int32_t lgn, int32_t pix, const double* R, int32_t (&src)[4],
                                                         double (&w)[4]) {
  int32_t ring, jp;
  knn_nest_to_ring(nside, lgn, pix, &ring, &jp);
  const KnnRing g = knn_ring(nside, ring);
  const double phi0 = knn_phi(g, jp);
  const double v0 = g.st * cos(phi0), v1 = g.st * sin(phi0), v2 = g.z;
  const double ux = R[0] * v0 + R[3] * v1 + R[6] * v2;
  const double uy = R[1] * v0 + R[4] * v1 + R[7] * v2;
  const double uz = R[2] * v0 + R[5] * v1 + R[8] * v2;
  const double s = sqrt(ux * ux + uy * uy);
  const double z = fmin(fmax(uz / sqrt(s * s + uz * uz), -1.0), 1.0);
  const double theta = atan2(s, uz);
  double phi = atan2(uy, ux);
  if (phi < 0.0) phi += 2.0 * M_PI;  // (a tiny negative phi becomes exactly 2 pi: interp_ring_pair wraps both positions)
  interp_stencil(nside, lgn, z, theta, phi, src, w);
}

// What a thread keeps of its pixel's stencil: rows of x (-1: a source outside the set, or no pixel at all) and float32 weights
struct RowStencil {
  int32_t row[4];
  float w[4];
};
__device__ __forceinline__ RowStencil row_stencil(int32_t nside, int32_t lgn, int64_t pix64, const double* __restrict__ R,
                                                  const int32_t* __restrict__ lut, int64_t M) {
  RowStencil s;
  const int64_t npix = (int64_t)12 * nside * nside;
  if (pix64 < 0 || pix64 >= npix) {  // (not a pixel: a row of zeros)
#pragma unroll
    for (int j = 0; j < 4; ++j) { s.row[j] = -1; s.w[j] = 0.0f; }
    return s;
  }
  int32_t src[4];
  double w[4];
  rotated_stencil(nside, lgn, (int32_t)pix64, R, src, w);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int32_t row = -1;
    if (src[j] >= 0 && src[j] < npix) row = lut ? lut[src[j]] : src[j];
    s.row[j] = row < M ? row : -1;  // (a table that names a row beyond the map is not followed)
    s.w[j] = (float)w[j];
  }
  return s;
}

// VEC channels of one output row: four gathers in flight, then the sum in the order of the stencil
template <int VEC>
__device__ __forceinline__ void gather4(const float* __restrict__ xm, const int32_t (&row)[4], const float (&w)[4], int64_t F, int c,
                                        float (&acc)[VEC]) {
  float a[4][VEC];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (row[j] >= 0) {
      ldv<VEC>(xm + (int64_t)row[j] * F + c, a[j]);
    } else {
#pragma unroll
      for (int v = 0; v < VEC; ++v) a[j][v] = 0.0f;
    }
  }
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc[v] = fmaf(w[3], a[3][v], fmaf(w[2], a[2][v], fmaf(w[1], a[1][v], w[0] * a[0][v])));
}

// Narrow rows: a lane owns a pixel.  F % VEC == 0, maps aligned to 4 VEC bytes.
template <int VEC>
__global__ __launch_bounds__(HI_BLOCK) void healpix_rotate_narrow_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t N,
                                                                         int32_t nside, int32_t lgn, int32_t F,
                                                                         const double* __restrict__ rot, int64_t n_rot,
                                                                         const int32_t* __restrict__ lut,
                                                                         const int64_t* __restrict__ indices, int64_t M) {
  const int64_t r = (int64_t)xcd_remap(blockIdx.x, gridDim.x) * HI_BLOCK + threadIdx.x;
  if (r >= M) return;  // (no barrier in this kernel)
  const int64_t pix = indices ? indices[r] : r;
  RowStencil s;
  for (int64_t n = blockIdx.y; n < N; n += gridDim.y) {
    if (n_rot > 1 || n == (int64_t)blockIdx.y) s = row_stencil(nside, lgn, pix, rot + (n_rot > 1 ? n * 9 : 0), lut, M);
    const float* xm = x + n * M * F;
    float* yr = y + (n * M + r) * F;
    for (int c = 0; c < F; c += VEC) {
      float acc[VEC];
      gather4<VEC>(xm, s.row, s.w, F, c, acc);
      stv<VEC>(yr + c, acc);
    }
  }
}

// Wide rows: stencils through LDS, lanes along the channels.
template <int VEC>
__global__ __launch_bounds__(HI_BLOCK) void healpix_rotate_wide_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t N,
                                                                       int32_t nside, int32_t lgn, int32_t F,
                                                                       const double* __restrict__ rot, int64_t n_rot,
                                                                       const int32_t* __restrict__ lut,
                                                                       const int64_t* __restrict__ indices, int64_t M) {
  __shared__ __attribute__((aligned(16))) int32_t srow[HI_BLOCK][4];
  __shared__ __attribute__((aligned(16))) float sw[HI_BLOCK][4];
  const int tid = (int)threadIdx.x;
  const int64_t r0 = (int64_t)xcd_remap(blockIdx.x, gridDim.x) * HI_BLOCK;
  const int npx = M - r0 < HI_BLOCK ? (int)(M - r0) : HI_BLOCK;  // >= 1: the grid holds ceil(M / HI_BLOCK) blocks
  const int64_t pix = tid < npx ? (indices ? indices[r0 + tid] : r0 + tid) : -1;
  const int Q = F / VEC, items = npx * Q;
  for (int64_t n = blockIdx.y; n < N; n += gridDim.y) {
    if (n_rot > 1 || n == (int64_t)blockIdx.y) {  // (uniform over the workgroup)
      __syncthreads();  // the previous sample's reads of the stencils are done
      if (tid < npx) {
        const RowStencil s = row_stencil(nside, lgn, pix, rot + (n_rot > 1 ? n * 9 : 0), lut, M);
#pragma unroll
        for (int j = 0; j < 4; ++j) { srow[tid][j] = s.row[j]; sw[tid][j] = s.w[j]; }
      }
      __syncthreads();
    }
    const float* xm = x + n * M * F;
    float* ym = y + (n * M + r0) * F;
    for (int i0 = tid; i0 < items; i0 += HI_BLOCK * HI_BATCH) {
      float acc[HI_BATCH][VEC];
#pragma unroll
      for (int u = 0; u < HI_BATCH; ++u) {
        const int i = i0 + u * HI_BLOCK;
        if (i < items) {
          const int px = i / Q, c = (i - px * Q) * VEC;
          gather4<VEC>(xm, srow[px], sw[px], F, c, acc[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < HI_BATCH; ++u) {
        const int i = i0 + u * HI_BLOCK;
        if (i < items) stv<VEC>(ym + (int64_t)i * VEC, acc[u]);  // (item i = VEC floats of the block's run of y)
      }
    }
  }
}

// The same stencils as a table: cols / vals [M, 4]; a source outside the set becomes (col = the row itself, val = 0)
__global__ __launch_bounds__(HI_BLOCK) void healpix_interp_table_kernel(int32_t nside, int32_t lgn, const double* __restrict__ rot,
                                                                        const int32_t* __restrict__ lut,
                                                                        const int64_t* __restrict__ indices, int64_t M,
                                                                        int32_t* __restrict__ cols, float* __restrict__ vals) {
  const int64_t r = (int64_t)blockIdx.x * HI_BLOCK + threadIdx.x;
  if (r >= M) return;
  const RowStencil s = row_stencil(nside, lgn, indices ? indices[r] : r, rot, lut, M);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    cols[r * 4 + j] = s.row[j] >= 0 ? s.row[j] : (int32_t)r;
    vals[r * 4 + j] = s.row[j] >= 0 ? s.w[j] : 0.0f;
  }
}

// the checks both entry points share: nside, the pixel set and its size
static int interp_set_ok(const char* who, int32_t nside, const int32_t* lut, const int64_t* indices, int64_t M) {
  if (nside < 1 || (nside & (nside - 1)) != 0) {
    set_error("%s: nside = %d is not a power of two >= 1", who, (int)nside);
    return DSPH_E_BADARG;
  }
  if (nside > HI_MAX_NSIDE) {
    set_error("%s: nside = %d; pixel indices are int32 here, which holds up to nside %d", who, (int)nside, HI_MAX_NSIDE);
    return DSPH_E_UNSUPPORTED;
  }
  const int64_t npix = (int64_t)12 * nside * nside;
  if ((indices == nullptr) != (lut == nullptr)) {
    set_error("%s: indices and lut come together (both NULL: the full sky)", who);
    return DSPH_E_BADARG;
  }
  if (!indices && M != npix) {
    set_error("%s: M = %lld rows without indices, the full sky of nside %d has %lld", who, (long long)M, (int)nside, (long long)npix);
    return DSPH_E_BADARG;
  }
  if (M < 0 || M > npix || M >= ((int64_t)1 << 31)) {
    set_error("%s: M = %lld rows outside [0, min(12 nside^2, 2^31 - 1)]", who, (long long)M);
    return DSPH_E_BADARG;
  }
  return DSPH_OK;
}

}  // namespace dsph

extern "C" {

// every argument is checked here, before any launch
int dsph_healpix_rotate(const float* x, float* y, int64_t N, int32_t nside, int32_t F, const double* rot, int64_t n_rot,
                        const int32_t* lut, const int64_t* indices, int64_t M, int device, void* hip_stream) {
  using namespace dsph;
  if (!x || !y || !rot) { set_error("healpix_rotate: NULL pointer (x, y and rot are required)"); return DSPH_E_BADARG; }
  const int rc = interp_set_ok("healpix_rotate", nside, lut, indices, M);
  if (rc != DSPH_OK) return rc;
  if (F < 1) { set_error("healpix_rotate: F = %d channels, must be at least 1", (int)F); return DSPH_E_BADARG; }
  if (N < 0) { set_error("healpix_rotate: negative batch N = %lld", (long long)N); return DSPH_E_BADARG; }
  if (n_rot != 1 && n_rot != N) {
    set_error("healpix_rotate: n_rot = %lld rotations for N = %lld maps (one for all, or one each)", (long long)n_rot, (long long)N);
    return DSPH_E_BADARG;
  }
  if (reinterpret_cast<uintptr_t>(rot) & 7) { set_error("healpix_rotate: rot is not 8-byte aligned"); return DSPH_E_BADARG; }
  const double elems = (double)N * (double)M * (double)F;
  if (elems >= 9.0e18 / 4) { set_error("healpix_rotate: N * M * F = %.3g elements do not fit 64-bit byte offsets", elems); return DSPH_E_UNSUPPORTED; }
  const size_t bytes = (size_t)(N * M * (int64_t)F) * sizeof(float);
  if (ranges_overlap(x, bytes, y, bytes)) {  // (maps of no bytes overlap nothing)
    set_error("healpix_rotate: x and y overlap; a gather cannot run in place");
    return DSPH_E_BADARG;
  }
  DeviceGuard guard(device);
  if (!select_device("healpix_rotate", device, guard)) return DSPH_E_HIP;
  if (N == 0 || M == 0) return DSPH_OK;
  hipStream_t stream = (hipStream_t)hip_stream;
  int lgn = 0;
  while ((1 << lgn) < nside) ++lgn;
  const int VEC = vec_width(F, ptr_bits({x, y}), true);
  const int64_t gx = (M + HI_BLOCK - 1) / HI_BLOCK;
  int64_t gy = std::min<int64_t>(N, HI_MAX_GRID_Y);
  // one rotation for the batch: a workgroup computes its stencils once and walks the samples with them, so y holds only as many
  // workgroups per block of pixels as it takes to fill the chip (measured at nside 1024, N 8, F 1: 3.35 ms with a workgroup per
  // sample, each computing the same stencils)
  if (n_rot == 1) gy = std::min(gy, std::max<int64_t>(1, (HI_FILL_GROUPS + gx - 1) / gx));
  const dim3 grid((unsigned)gx, (unsigned)gy);
  if (F >= HI_WIDE_F) {
    DSPH_LAUNCH_BY_VEC(VEC, healpix_rotate_wide_kernel, grid, dim3(HI_BLOCK), stream, x, y, N, nside, (int32_t)lgn, F, rot, n_rot, lut,
                       indices, M);
  } else {
    DSPH_LAUNCH_BY_VEC(VEC, healpix_rotate_narrow_kernel, grid, dim3(HI_BLOCK), stream, x, y, N, nside, (int32_t)lgn, F, rot, n_rot, lut,
                       indices, M);
  }
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

int dsph_healpix_interp_table(int32_t nside, const double* rot, const int32_t* lut, const int64_t* indices, int64_t M, int32_t* cols,
                              float* vals, int device, void* hip_stream) {
  using namespace dsph;
  if (!rot || !cols || !vals) { set_error("healpix_interp_table: NULL pointer (rot, cols and vals are required)"); return DSPH_E_BADARG; }
  const int rc = interp_set_ok("healpix_interp_table", nside, lut, indices, M);
  if (rc != DSPH_OK) return rc;
  if (reinterpret_cast<uintptr_t>(rot) & 7) { set_error("healpix_interp_table: rot is not 8-byte aligned"); return DSPH_E_BADARG; }
  DeviceGuard guard(device);
  if (!select_device("healpix_interp_table", device, guard)) return DSPH_E_HIP;
  if (M == 0) return DSPH_OK;
  hipStream_t stream = (hipStream_t)hip_stream;
  int lgn = 0;
  while ((1 << lgn) < nside) ++lgn;
  hipLaunchKernelGGL(healpix_interp_table_kernel, dim3((unsigned)((M + HI_BLOCK - 1) / HI_BLOCK)), dim3(HI_BLOCK), 0, stream, nside,
                     (int32_t)lgn, rot, lut, indices, M, cols, vals);
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

}  // extern "C"
