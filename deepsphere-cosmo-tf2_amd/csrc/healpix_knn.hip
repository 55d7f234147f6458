// The k nearest pixels of every pixel of a (partial) HEALPix map, by chord distance between pixel centres in float64: the neighbour
// search behind the reference's SphereHealpix(k = n_neighbors) graphs (healpix.healpix_graph(mode="knn") does it on the host with
// a k-d tree over all pixel centres; healpix.healpix_laplacian_ell builds the graph from this kernel's result on the device).
//
// One wave per pixel.  The candidates are a window in the RING scheme around the pixel's own ring ir and position: the rings
// ir - R .. ir + R that exist, and on each of them the 2 P + 1 positions nearest in phi (the whole ring where it is no longer than
// that).  A ring's z and phi step are closed-form (healpix.pix2vec), so the window needs no handling of face borders; a candidate
// (ring, position) becomes a NEST id by the (face, ix, iy) arithmetic of healpix.ring2nest and a row through `lut`.  Every lane
// holds up to KNN_SLOTS candidates (squared chord, row) in registers; k rounds of a wave-wide arg-min on (d2, row) pick the
// neighbours in ascending order.  No LDS, no scratch memory.
//
// What lies outside the window is bounded from below by distances the wave evaluates like candidates ("guards"):
//   * the first ring left out on either side, at the pixel's own phi: the chord of the colatitude difference, below which no
//     point of that ring or of any ring beyond it can lie;
//   * on every ring of the window that is not taken whole, the first position left out on either side: on a ring d2 grows with
//     |dphi| up to pi, and the positions left out form one arc that does not contain the pixel's phi.
// ok = 1 iff k candidates of the set were found and the k-th squared chord is below the smallest guard: then no pixel outside the
// window can belong to the k nearest.  Rows with ok = 0 are the caller's to complete (the edge of a survey footprint, where the
// k-th neighbour lies further out than the window reaches).
//
// (R, P) by k: knn_window() below; the table was sized on the full sky, where every row must come out ok.
#include <algorithm>
#include <cmath>

#include "dsphere_common.h"
#include "healpix_ring.h"

namespace dsph {

constexpr int KNN_THREADS = 256;       // four waves, four pixels per trip of a workgroup
constexpr int KNN_SLOTS = 4;           // candidates a lane holds: three registers each
constexpr int KNN_MAX_K = 64;          // lane r keeps the r-th neighbour until the row is stored
constexpr int KNN_MAX_NSIDE = 8192;    // 12 nside^2 - 1 fits int32 up to here
constexpr int KNN_MAX_GRID = 1 << 20;  // workgroups; further rows on further trips

struct KnnWindow {
  int R, P;
};
// The window for k neighbours.  Sized on the full sky (every pixel of nside 1 .. 256 ok, by the host model of this file's
// arithmetic), smallest first; the guards decide per row, so a window that is too small costs ok flags, never a wrong row.
inline KnnWindow knn_window(int k) {
  if (k <= 8) return {3, 3};
  if (k <= 20) return {5, 5};
  if (k <= 40) return {7, 7};
  return {7, 8};
}
inline int knn_window_candidates(const KnnWindow& w) { return (2 * w.R + 1) * (2 * w.P + 1); }

// What a wave knows of its pixel
struct KnnPixel {
  int32_t nside, lgn, R, P, ring, row;
  double phi;
  double v[3];
};
__host__ __device__ __forceinline__ KnnPixel knn_pixel(int32_t nside, int32_t lgn, int32_t R, int32_t P, int32_t pix, int32_t row) {
  KnnPixel px;
  px.nside = nside; px.lgn = lgn; px.R = R; px.P = P; px.row = row;
  int32_t jp;
  knn_nest_to_ring(nside, lgn, pix, &px.ring, &jp);
  const KnnRing g = knn_ring(nside, px.ring);
  px.phi = knn_phi(g, jp);
  px.v[0] = g.st * cos(px.phi); px.v[1] = g.st * sin(px.phi); px.v[2] = g.z;
  return px;
}

// Candidate c < (2 R + 1)(2 P + 1) of the window: ring index c / (2 P + 1), place c % (2 P + 1).  -> false where the window has
// nothing there (a ring beyond a pole, a place beyond the end of a short ring); else the candidate's NEST id and squared chord.
__host__ __device__ __forceinline__ bool knn_candidate(const KnnPixel& px, int32_t c, int32_t* nest, double* d2) {
  const int32_t wp = 2 * px.P + 1;
  const int32_t ri = c / wp, q = c - ri * wp;
  const int32_t ring = px.ring - px.R + ri;
  if (ring < 1 || ring > 4 * px.nside - 1) return false;
  const KnnRing g = knn_ring(px.nside, ring);
  const int32_t n4 = 4 * g.nr;
  int32_t jp;
  if (n4 <= wp) {
    if (q >= n4) return false;
    jp = q + 1;
  } else {
    jp = knn_wrap(knn_centre(g, px.phi) + q - px.P, n4);
  }
  *nest = knn_ring_to_nest(px.nside, px.lgn, ring, g.nr, g.kshift, jp);
  *d2 = knn_d2(g, knn_phi(g, jp), px.v);
  return true;
}
// Guard b < 2 (2 R + 1) + 2 of the window: b < 2 (2 R + 1): the first position left out of ring index b / 2 on side b % 2;
// the last two: the first ring left out on either side, at the pixel's phi.  -> false where nothing is left out there.
__host__ __device__ __forceinline__ bool knn_guard(const KnnPixel& px, int32_t b, double* d2) {
  const int32_t nrings = 2 * px.R + 1, wp = 2 * px.P + 1;
  if (b >= 2 * nrings) {
    const int32_t ring = b == 2 * nrings ? px.ring - px.R - 1 : px.ring + px.R + 1;
    if (ring < 1 || ring > 4 * px.nside - 1) return false;
    *d2 = knn_d2(knn_ring(px.nside, ring), px.phi, px.v);
    return true;
  }
  const int32_t ring = px.ring - px.R + (b >> 1);
  if (ring < 1 || ring > 4 * px.nside - 1) return false;
  const KnnRing g = knn_ring(px.nside, ring);
  const int32_t n4 = 4 * g.nr;
  if (n4 <= wp) return false;  // taken whole
  const int32_t jp = knn_wrap(knn_centre(g, px.phi) + ((b & 1) ? px.P + 1 : -px.P - 1), n4);
  *d2 = knn_d2(g, knn_phi(g, jp), px.v);
  return true;
}
constexpr int KNN_MAX_GUARDS = 64;  // 2 (2 R + 1) + 2 <= 64: one per lane

__device__ __forceinline__ void knn_wave_argmin(double& d, int32_t& r) {  // every lane ends with the wave's smallest (d, r)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double od = __shfl_xor(d, off, 64);
    const int32_t orow = __shfl_xor(r, off, 64);
    if (od < d || (od == d && orow < r)) { d = od; r = orow; }
  }
}

__global__ __launch_bounds__(KNN_THREADS) void healpix_knn_kernel(int32_t nside, int32_t lgn, int32_t k, int32_t R, int32_t P,
                                                                  const int64_t* __restrict__ indices, const int32_t* __restrict__ lut,
                                                                  int64_t M, int32_t* __restrict__ nbr, double* __restrict__ d2out,
                                                                  uint8_t* __restrict__ ok) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int32_t npix = 12 * nside * nside;
  const int32_t ncand = (2 * R + 1) * (2 * P + 1), nguard = 2 * (2 * R + 1) + 2;
  const double inf = __builtin_huge_val();
  for (int64_t row = (int64_t)blockIdx.x * (KNN_THREADS / 64) + wave; row < M; row += (int64_t)gridDim.x * (KNN_THREADS / 64)) {
    const int64_t pix64 = indices ? indices[row] : row;
    if (pix64 < 0 || pix64 >= npix) {  // (not a pixel: the wave has nothing to measure from)
      if (lane < k) { nbr[row * k + lane] = -1; d2out[row * k + lane] = inf; }
      if (lane == 0) ok[row] = 0;
      continue;
    }
    const KnnPixel px = knn_pixel(nside, lgn, R, P, (int32_t)pix64, (int32_t)row);
    double cd[KNN_SLOTS];
    int32_t cr[KNN_SLOTS];
#pragma unroll
    for (int s = 0; s < KNN_SLOTS; ++s) {
      cd[s] = inf; cr[s] = INT32_MAX;
      const int32_t c = lane + 64 * s;
      int32_t nest;
      double d;
      if (c < ncand && knn_candidate(px, c, &nest, &d) && nest >= 0 && nest < npix) {
        const int32_t r = lut ? lut[nest] : nest;
        if (r >= 0 && r != px.row) { cd[s] = d; cr[s] = r; }
      }
    }
    double bound = inf;
    {
      double d;
      if (lane < nguard && knn_guard(px, lane, &d)) bound = d;
      int32_t unused = 0;
      knn_wave_argmin(bound, unused);
    }
    double rd = inf, kd = inf;  // this lane's neighbour (lane r: the r-th), the k-th distance
    int32_t rr = -1;
    bool found = true;
    for (int32_t r = 0; r < k; ++r) {
      double bd = cd[0];
      int32_t br = cr[0];
#pragma unroll
      for (int s = 1; s < KNN_SLOTS; ++s)
        if (cd[s] < bd || (cd[s] == bd && cr[s] < br)) { bd = cd[s]; br = cr[s]; }
      knn_wave_argmin(bd, br);
      if (br == INT32_MAX) { found = false; break; }  // (wave-uniform: the window holds fewer than k pixels of the set)
#pragma unroll
      for (int s = 0; s < KNN_SLOTS; ++s)
        if (cr[s] == br) { cd[s] = inf; cr[s] = INT32_MAX; }
      if (lane == r) { rd = bd; rr = br; }
      kd = bd;
    }
    if (lane < k) { nbr[row * k + lane] = rr; d2out[row * k + lane] = rd; }
    if (lane == 0) ok[row] = (found && kd < bound) ? 1 : 0;
  }
}

}  // namespace dsph

extern "C" {

// every argument is checked here, before any launch
int dsph_healpix_knn(int32_t nside, int32_t k, const int64_t* indices, const int32_t* lut, int64_t M, int32_t* nbr, double* d2,
                     uint8_t* ok, int device, void* hip_stream) {
  using namespace dsph;
  if (!nbr || !d2 || !ok) { set_error("healpix_knn: NULL pointer (nbr, d2 and ok are required)"); return DSPH_E_BADARG; }
  if (nside < 1 || (nside & (nside - 1)) != 0) {
    set_error("healpix_knn: nside = %d is not a power of two >= 1", (int)nside);
    return DSPH_E_BADARG;
  }
  if (nside > KNN_MAX_NSIDE) {
    set_error("healpix_knn: nside = %d; pixel indices are int32 here, which holds up to nside %d", (int)nside, KNN_MAX_NSIDE);
    return DSPH_E_UNSUPPORTED;
  }
  if (k < 1) { set_error("healpix_knn: k = %d neighbours, must be at least 1", (int)k); return DSPH_E_BADARG; }
  if (k > KNN_MAX_K) { set_error("healpix_knn: k = %d neighbours; a wave keeps at most %d", (int)k, KNN_MAX_K); return DSPH_E_UNSUPPORTED; }
  const int64_t npix = (int64_t)12 * nside * nside;
  if ((indices == nullptr) != (lut == nullptr)) {
    set_error("healpix_knn: indices and lut come together (both NULL: the full sky)");
    return DSPH_E_BADARG;
  }
  if (!indices && M != npix) {
    set_error("healpix_knn: M = %lld rows without indices, the full sky of nside %d has %lld", (long long)M, (int)nside, (long long)npix);
    return DSPH_E_BADARG;
  }
  if (M < 0 || M > npix || M >= ((int64_t)1 << 31)) {
    set_error("healpix_knn: M = %lld rows outside [0, min(12 nside^2, 2^31 - 1)]", (long long)M);
    return DSPH_E_BADARG;
  }
  if (M <= k) {
    set_error("healpix_knn: a set of M = %lld pixels has no %d neighbours per pixel (M > k is required)", (long long)M, (int)k);
    return DSPH_E_BADARG;
  }
  const KnnWindow w = knn_window(k);
  if (knn_window_candidates(w) > 64 * KNN_SLOTS || 2 * (2 * w.R + 1) + 2 > KNN_MAX_GUARDS) {
    set_error("healpix_knn: the window for k = %d does not fit a wave", (int)k);
    return DSPH_E_UNSUPPORTED;
  }
  DeviceGuard guard(device);
  if (!guard.ok) { set_error("healpix_knn: cannot select device %d", device); return DSPH_E_HIP; }
  hipStream_t stream = (hipStream_t)hip_stream;
  int lgn = 0;
  while ((1 << lgn) < nside) ++lgn;
  const int64_t groups = (M + KNN_THREADS / 64 - 1) / (KNN_THREADS / 64);
  const dim3 grid((unsigned)std::min<int64_t>(groups, KNN_MAX_GRID));
  hipLaunchKernelGGL(healpix_knn_kernel, grid, dim3(KNN_THREADS), 0, stream, nside, (int32_t)lgn, k, (int32_t)w.R, (int32_t)w.P, indices,
                     lut, M, nbr, d2, ok);
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

}  // extern "C"
