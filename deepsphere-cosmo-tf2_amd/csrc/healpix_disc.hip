// The kernel matrix of HealpySmoothing built on the device: how many pixels of a (partial) HEALPix map lie within a disc around
// every pixel (dsph_healpix_disc_count: the largest count is the row width W of the layer's table), and the finished table -- the W
// nearest pixels of every pixel by float64 chord distance, their Gaussian weights, normalised, every row ordered by column
// (dsph_healpix_gauss_table).  The host does the same with a k-d tree over all pixel centres and numpy (HealpySmoothing._build_tree,
// _finish_table).
//
// One workgroup per pixel.  The candidates are a window in the RING scheme (healpix_ring.h) sized from a reach rho: the rings whose
// colatitude can lie within rho of the pixel's, one more on either side, and on each of them the positions whose phi can lie within
// rho of the pixel, one more on either side (the whole ring where that is all of it).  Groups of DISC_GROUP lanes take one ring
// each.  What lies outside the window is bounded from below by the guards of healpix_knn.hip, evaluated like candidates: the first
// ring left out on either side at the pixel's own phi, and the first position left out on either side of every ring not taken whole.
// The window's arithmetic only decides how tight the window is; whether a row is guaranteed is decided by the guards alone.
//
// The count kernel keeps nothing: every lane counts its candidates within r2, the workgroup adds up in LDS.  ok = 1 iff every
// guard lies beyond r2.
// The table kernel files the candidates of the set as (d2, row) in LDS, ranks every candidate by counting the candidates before
// it in the order (d2, row) -- a total order, so the result does not depend on where a candidate was filed -- keeps ranks below W,
// ranks those by row for the column order, sums the float32 weights in float64 in a fixed order and stores the row.  ok = 1 iff
// W candidates were found and the W-th squared chord lies below the smallest guard.  The window reaches DISC_MARGIN rho.
// No global atomics (LDS atomics only), no scratch memory, every element written by one thread.
#include <algorithm>
#include <cmath>

#include "dsphere_common.h"
#include "healpix_ring.h"

namespace dsph {

constexpr int DISC_THREADS = 256;        // one workgroup per row
constexpr int DISC_GROUP = 16;           // lanes that share a ring of the window
constexpr int DISC_MAX_NSIDE = 8192;     // 12 nside^2 - 1 fits int32 up to here
constexpr int DISC_MAX_W = 512;          // entries of a row
constexpr int DISC_MAX_CAND = 2048;      // candidates of a row in LDS: 12 bytes each
constexpr int DISC_MAX_GRID = 1 << 16;   // workgroups; further rows on further trips
constexpr double DISC_MARGIN = 1.125;    // the table's window reaches this times rho (the W-th neighbour lies within 1.08 rho on
                                         // the full sky); a window that is too small costs ok flags, never a wrong row
// LDS of the table kernel: candidates 24 KiB + selection 6 KiB, so that five workgroups fit the 160 KiB of a CU (the registers
// of the float64 sin / cos / acos / asin / exp allow two: 217 VGPRs, no scratch)
static_assert(5 * (DISC_MAX_CAND * 12 + DISC_MAX_W * 12 + 64) <= 160 * 1024, "several rows per CU");

// What a workgroup knows of its pixel
struct DiscPixel {
  int32_t nside, lgn, ring;
  double phi, colat;
  double v[3];
};
__host__ __device__ __forceinline__ DiscPixel disc_pixel(int32_t nside, int32_t lgn, int32_t pix) {
  DiscPixel px;
  px.nside = nside; px.lgn = lgn;
  int32_t jp;
  knn_nest_to_ring(nside, lgn, pix, &px.ring, &jp);
  const KnnRing g = knn_ring(nside, px.ring);
  px.phi = knn_phi(g, jp);
  px.colat = atan2(g.st, g.z);
  px.v[0] = g.st * cos(px.phi); px.v[1] = g.st * sin(px.phi); px.v[2] = g.z;
  return px;
}
// the (real-valued) ring number at height z: the inverse of knn_ring's z
__host__ __device__ __forceinline__ double disc_ring_of_z(int32_t nside, double z) {
  const double n = (double)nside;
  if (z > 2.0 / 3.0) return n * sqrt(fmax(0.0, 3.0 * (1.0 - z)));
  if (z < -2.0 / 3.0) return 4.0 * n - n * sqrt(fmax(0.0, 3.0 * (1.0 + z)));
  return 2.0 * n - 1.5 * n * z;
}
// The rings of the window for a reach (radians, <= pi) around colatitude `colat`, own ring `ring`: one more than can hold a point
// within the reach on either side, never fewer than the pixel's own ring
__host__ __device__ __forceinline__ void disc_ring_range(int32_t nside, int32_t ring, double colat, double reach, int32_t* first,
                                                         int32_t* last) {
  const int32_t nrings = 4 * nside - 1;
  const double lo = colat - reach, hi = colat + reach;
  int32_t a = 1, b = nrings;
  if (lo > 0.0) a = (int32_t)floor(disc_ring_of_z(nside, cos(lo))) - 1;
  if (hi < M_PI) b = (int32_t)ceil(disc_ring_of_z(nside, cos(hi))) + 1;
  a = a < ring ? a : ring; b = b > ring ? b : ring;
  *first = a < 1 ? 1 : a; *last = b > nrings ? nrings : b;
}
// Positions of ring g on either side of the one nearest to the pixel's phi that the window takes: one more than can lie within the
// squared chord r2w of a pixel at height z0, sin(theta) st0; -1: the whole ring
__host__ __device__ __forceinline__ int32_t disc_half_width(const KnnRing& g, double z0, double st0, double r2w) {
  const double dz = g.z - z0;
  const double den = 2.0 * g.st * st0;
  const double c = (g.st * g.st + st0 * st0 + dz * dz - r2w) / den;  // cos of the largest |dphi| inside (den > 0: no centre at a pole)
  if (!(c > -1.0)) return -1;
  const double dphi = c >= 1.0 ? 0.0 : acos(c);
  const double p = ceil(dphi / g.step) + 1.0;
  if (2.0 * p + 1.0 >= (double)(4 * g.nr)) return -1;
  return (int32_t)p;
}
__host__ __device__ __forceinline__ double disc_r2(double reach) {  // squared chord of an angle
  const double s = 2.0 * sin(0.5 * reach);
  return s * s;
}

// Host: the most candidates a window of this reach holds, over the pixels of every ring (a window depends on the pixel's ring
// only); two positions per ring on top, for a half width that the device rounds the other way.  Stops counting beyond `cap`.
static int64_t disc_max_candidates(int32_t nside, double reach, int64_t cap) {
  const double r2w = disc_r2(reach);
  int64_t worst = 0;
  for (int32_t ring = 1; ring <= 2 * nside; ++ring) {  // (the southern half mirrors the northern)
    const KnnRing g0 = knn_ring(nside, ring);
    int32_t first, last;
    disc_ring_range(nside, ring, atan2(g0.st, g0.z), reach, &first, &last);
    int64_t n = 0;
    for (int32_t r = first; r <= last && n <= cap; ++r) {
      const KnnRing g = knn_ring(nside, r);
      const int32_t P = disc_half_width(g, g0.z, g0.st, r2w);
      n += P < 0 ? 4 * g.nr : std::min(2 * P + 3, 4 * g.nr);
    }
    worst = std::max(worst, n);
    if (worst > cap) break;
  }
  return worst;
}

// The window of pixel px for a reach, ring by ring: cand(nest, d2) for every position taken, by the lanes of the ring's group;
// this is thread `tid`'s share.  -> the thread's smallest guard (squared chord); the workgroup's bound is the minimum over its threads.
template <class Cand>
__host__ __device__ __forceinline__ double disc_scan(const DiscPixel& px, double reach, int tid, Cand&& cand) {
  const int sub = tid / DISC_GROUP, l = tid % DISC_GROUP;
  constexpr int NSUB = DISC_THREADS / DISC_GROUP;
  const double r2w = disc_r2(reach);
  const double st0 = sqrt(px.v[0] * px.v[0] + px.v[1] * px.v[1]);
  double bound = __builtin_huge_val();
  int32_t first, last;
  disc_ring_range(px.nside, px.ring, px.colat, reach, &first, &last);
  if (tid < 2) {  // the first ring left out on either side, at the pixel's phi
    const int32_t ring = tid == 0 ? first - 1 : last + 1;
    if (ring >= 1 && ring <= 4 * px.nside - 1) bound = knn_d2(knn_ring(px.nside, ring), px.phi, px.v);
  }
  for (int32_t ring = first + sub; ring <= last; ring += NSUB) {
    const KnnRing g = knn_ring(px.nside, ring);
    const int32_t n4 = 4 * g.nr;
    const int32_t P = disc_half_width(g, px.v[2], st0, r2w);
    const int32_t jc = knn_centre(g, px.phi);
    const int32_t cnt = P < 0 ? n4 : 2 * P + 1;
    if (P >= 0 && l < 2) {  // the first position left out on either side
      const int32_t jp = knn_wrap(jc + (l ? P + 1 : -P - 1), n4);
      bound = fmin(bound, knn_d2(g, knn_phi(g, jp), px.v));
    }
    for (int32_t q = l; q < cnt; q += DISC_GROUP) {
      const int32_t jp = P < 0 ? q + 1 : knn_wrap(jc - P + q, n4);
      cand(knn_ring_to_nest(px.nside, px.lgn, ring, g.nr, g.kshift, jp), knn_d2(g, knn_phi(g, jp), px.v));
    }
  }
  return bound;
}

// every thread ends with the workgroup's minimum; `slots`: DISC_THREADS / 64 doubles of LDS (a barrier inside, before and after)
__device__ __forceinline__ double disc_block_min(double v, double* slots) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
  __syncthreads();
  if (((int)threadIdx.x & 63) == 0) slots[(int)threadIdx.x >> 6] = v;
  __syncthreads();
  double m = slots[0];
#pragma unroll
  for (int w = 1; w < DISC_THREADS / 64; ++w) m = fmin(m, slots[w]);
  return m;
}

__global__ __launch_bounds__(DISC_THREADS) void healpix_disc_count_kernel(int32_t nside, int32_t lgn, double reach, double r2,
                                                                          const int64_t* __restrict__ indices,
                                                                          const int32_t* __restrict__ lut, int64_t M,
                                                                          int32_t* __restrict__ count, uint8_t* __restrict__ ok) {
  __shared__ double s_min[DISC_THREADS / 64];
  __shared__ int32_t s_count;
  const int32_t npix = 12 * nside * nside;
  for (int64_t row = blockIdx.x; row < M; row += gridDim.x) {
    const int64_t pix64 = indices ? indices[row] : row;
    if (pix64 < 0 || pix64 >= npix) {  // (not a pixel: nothing to measure from)
      if (threadIdx.x == 0) { count[row] = 0; ok[row] = 0; }
      continue;
    }
    if (threadIdx.x == 0) s_count = 0;
    const DiscPixel px = disc_pixel(nside, lgn, (int32_t)pix64);
    int32_t mine = 0;
    double bound = disc_scan(px, reach, (int)threadIdx.x, [&](int32_t nest, double d2) {
      if (d2 <= r2 && nest >= 0 && nest < npix && (lut ? lut[nest] >= 0 : true)) ++mine;
    });
    bound = disc_block_min(bound, s_min);  // (its barriers order the reset of s_count before the adds)
    if (mine) atomicAdd(&s_count, mine);
    __syncthreads();
    if (threadIdx.x == 0) { count[row] = s_count; ok[row] = bound > r2 ? 1 : 0; }
    __syncthreads();
  }
}

__global__ __launch_bounds__(DISC_THREADS) void healpix_gauss_table_kernel(int32_t nside, int32_t lgn, int32_t W, double reach,
                                                                           double sigma, const int64_t* __restrict__ indices,
                                                                           const int32_t* __restrict__ lut, int64_t M,
                                                                           int32_t* __restrict__ cols, float* __restrict__ vals,
                                                                           float* __restrict__ raw, uint8_t* __restrict__ ok) {
  __shared__ double s_d[DISC_MAX_CAND];    // candidates: squared chord ...
  __shared__ int32_t s_r[DISC_MAX_CAND];   // ... and row; after the selection: the row's columns
  __shared__ double s_sd[DISC_MAX_W];      // the W nearest by rank: squared chord ...
  __shared__ int32_t s_sr[DISC_MAX_W];     // ... and row
  __shared__ double s_min[DISC_THREADS / 64];
  __shared__ double s_dw, s_sum;
  __shared__ int32_t s_n;
  float* const s_v = reinterpret_cast<float*>(s_d);  // after the selection: the row's values (the candidates are dead by then)
  const int tid = (int)threadIdx.x;
  const int32_t npix = 12 * nside * nside;
  const double a = -0.5 / (sigma * sigma);  // the host's kernel_func: exp(-0.5 / sigma^2 * theta^2)
  for (int64_t row = blockIdx.x; row < M; row += gridDim.x) {
    const int64_t base = row * (int64_t)W;
    const int64_t pix64 = indices ? indices[row] : row;
    if (pix64 < 0 || pix64 >= npix) {  // (not a pixel: nothing to measure from)
      for (int32_t j = tid; j < W; j += DISC_THREADS) {
        cols[base + j] = -1; vals[base + j] = 0.f;
        if (raw) raw[base + j] = 0.f;
      }
      if (tid == 0) ok[row] = 0;
      continue;
    }
    if (tid == 0) s_n = 0;
    __syncthreads();
    const DiscPixel px = disc_pixel(nside, lgn, (int32_t)pix64);
    double bound = disc_scan(px, reach, (int)threadIdx.x, [&](int32_t nest, double d2) {
      if (nest < 0 || nest >= npix) return;
      const int32_t r = lut ? lut[nest] : nest;
      if (r < 0) return;
      const int32_t slot = atomicAdd(&s_n, 1);
      if (slot < DISC_MAX_CAND) { s_d[slot] = d2; s_r[slot] = r; }
    });
    bound = disc_block_min(bound, s_min);  // (barriers: the candidates and s_n are in LDS)
    const int32_t n = s_n;
    if (n < W || n > DISC_MAX_CAND) {  // (workgroup-uniform) too few pixels of the set in the window, or more than LDS holds
      for (int32_t j = tid; j < W; j += DISC_THREADS) {
        cols[base + j] = -1; vals[base + j] = 0.f;
        if (raw) raw[base + j] = 0.f;
      }
      if (tid == 0) ok[row] = 0;
      __syncthreads();
      continue;
    }
    // the W smallest by (d2, row): a candidate's rank is the number of candidates before it
    for (int32_t i = tid; i < n; i += DISC_THREADS) {
      const double di = s_d[i];
      const int32_t ri = s_r[i];
      int32_t rank = 0;
      for (int32_t j = 0; j < n; ++j) {
        const double dj = s_d[j];
        rank += (dj < di || (dj == di && s_r[j] < ri)) ? 1 : 0;
      }
      if (rank < W) { s_sd[rank] = di; s_sr[rank] = ri; }
      if (rank == W - 1) s_dw = di;
    }
    __syncthreads();
    // by column; the weight in float64, rounded to float32
    for (int32_t i = tid; i < W; i += DISC_THREADS) {
      const int32_t ri = s_sr[i];
      int32_t pos = 0;
      for (int32_t j = 0; j < W; ++j) pos += s_sr[j] < ri ? 1 : 0;
      const double theta = 2.0 * asin(fmin(0.5 * sqrt(s_sd[i]), 1.0));
      s_r[pos] = ri;
      s_v[pos] = (float)exp(a * (theta * theta));
    }
    __syncthreads();
    // the float64 sum of the float32 weights, ascending by column within a lane's piece, the pieces by a fixed tree
    if (tid < 64) {
      const int32_t per = (W + 63) / 64;
      double s = 0.0;
      for (int32_t j = tid * per; j < (tid + 1) * per && j < W; ++j) s += (double)s_v[j];
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) s += __shfl_xor(s, off, 64);
      if (tid == 0) s_sum = s;
    }
    __syncthreads();
    const double sum = s_sum;
    for (int32_t j = tid; j < W; j += DISC_THREADS) {
      const float v = s_v[j];
      cols[base + j] = s_r[j];
      vals[base + j] = (float)((double)v / sum);
      if (raw) raw[base + j] = v;
    }
    if (tid == 0) ok[row] = s_dw < bound ? 1 : 0;
    __syncthreads();
  }
}

// the argument checks the two entry points share; `what`: the name in the messages
static int disc_check(const char* what, int32_t nside, const int64_t* indices, const int32_t* lut, int64_t M) {
  if (nside < 1 || (nside & (nside - 1)) != 0) {
    set_error("%s: nside = %d is not a power of two >= 1", what, (int)nside);
    return DSPH_E_BADARG;
  }
  if (nside > DISC_MAX_NSIDE) {
    set_error("%s: nside = %d; pixel indices are int32 here, which holds up to nside %d", what, (int)nside, DISC_MAX_NSIDE);
    return DSPH_E_UNSUPPORTED;
  }
  const int64_t npix = (int64_t)12 * nside * nside;
  if ((indices == nullptr) != (lut == nullptr)) {
    set_error("%s: indices and lut come together (both NULL: the full sky)", what);
    return DSPH_E_BADARG;
  }
  if (!indices && M != npix) {
    set_error("%s: M = %lld rows without indices, the full sky of nside %d has %lld", what, (long long)M, (int)nside, (long long)npix);
    return DSPH_E_BADARG;
  }
  if (M < 1 || M > npix || M >= ((int64_t)1 << 31)) {
    set_error("%s: M = %lld rows outside [1, min(12 nside^2, 2^31 - 1)]", what, (long long)M);
    return DSPH_E_BADARG;
  }
  return DSPH_OK;
}

}  // namespace dsph

extern "C" {

// every argument is checked here, before any launch
int dsph_healpix_disc_count(int32_t nside, double r2, const int64_t* indices, const int32_t* lut, int64_t M, int32_t* count,
                            uint8_t* ok, int device, void* hip_stream) {
  using namespace dsph;
  if (!count || !ok) { set_error("healpix_disc_count: NULL pointer (count and ok are required)"); return DSPH_E_BADARG; }
  if (const int rc = disc_check("healpix_disc_count", nside, indices, lut, M)) return rc;
  if (!(r2 >= 0.0 && r2 <= 4.0)) {
    set_error("healpix_disc_count: r2 = %g is not the squared chord of a radius in [0, pi]", r2);
    return DSPH_E_BADARG;
  }
  DeviceGuard guard(device);
  if (!guard.ok) { set_error("healpix_disc_count: cannot select device %d", device); return DSPH_E_HIP; }
  int lgn = 0;
  while ((1 << lgn) < nside) ++lgn;
  const double reach = 2.0 * asin(fmin(0.5 * sqrt(r2), 1.0));
  const dim3 grid((unsigned)std::min<int64_t>(M, DISC_MAX_GRID));
  hipLaunchKernelGGL(healpix_disc_count_kernel, grid, dim3(DISC_THREADS), 0, (hipStream_t)hip_stream, nside, (int32_t)lgn, reach, r2,
                     indices, lut, M, count, ok);
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

int dsph_healpix_gauss_table(int32_t nside, int32_t W, double sigma_rad, double rho, const int64_t* indices, const int32_t* lut,
                             int64_t M, int32_t* cols, float* vals, float* raw, uint8_t* ok, int device, void* hip_stream) {
  using namespace dsph;
  if (!cols || !vals || !ok) {
    set_error("healpix_gauss_table: NULL pointer (cols, vals and ok are required; raw may be NULL)");
    return DSPH_E_BADARG;
  }
  if (const int rc = disc_check("healpix_gauss_table", nside, indices, lut, M)) return rc;
  if (W < 1) { set_error("healpix_gauss_table: W = %d entries per row, must be at least 1", (int)W); return DSPH_E_BADARG; }
  if (W > DISC_MAX_W) {
    set_error("healpix_gauss_table: W = %d entries per row; a workgroup selects at most %d", (int)W, DISC_MAX_W);
    return DSPH_E_UNSUPPORTED;
  }
  if (M < W) {
    set_error("healpix_gauss_table: a set of M = %lld pixels has no rows of W = %d (M >= W is required)", (long long)M, (int)W);
    return DSPH_E_BADARG;
  }
  if (!(sigma_rad > 0.0) || !(rho > 0.0) || !(rho <= M_PI)) {
    set_error("healpix_gauss_table: sigma_rad = %g, rho = %g: sigma_rad > 0 and 0 < rho <= pi are required", sigma_rad, rho);
    return DSPH_E_BADARG;
  }
  const double reach = fmin(DISC_MARGIN * rho, M_PI);
  const int64_t need = disc_max_candidates(nside, reach, DISC_MAX_CAND);
  if (need > DISC_MAX_CAND) {
    set_error("healpix_gauss_table: the window for rho = %g at nside %d holds more than the %d candidates of a workgroup's LDS", rho,
              (int)nside, DISC_MAX_CAND);
    return DSPH_E_UNSUPPORTED;
  }
  DeviceGuard guard(device);
  if (!guard.ok) { set_error("healpix_gauss_table: cannot select device %d", device); return DSPH_E_HIP; }
  int lgn = 0;
  while ((1 << lgn) < nside) ++lgn;
  const dim3 grid((unsigned)std::min<int64_t>(M, DISC_MAX_GRID));
  hipLaunchKernelGGL(healpix_gauss_table_kernel, grid, dim3(DISC_THREADS), 0, (hipStream_t)hip_stream, nside, (int32_t)lgn, W, reach,
                     sigma_rad, indices, lut, M, cols, vals, raw, ok);
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

}  // extern "C"
