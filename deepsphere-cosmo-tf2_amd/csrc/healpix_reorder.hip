// RING <-> NEST reordering of full-sky HEALPix maps (the reference's workflow around HealpyGCNN: hp.reorder(m, r2n=True) on the way in,
// n2r=True on the way out; healpy_layers.HealpyReorder here).  A permutation of rows: byte work, nothing is computed but addresses.
//
// Both directions walk aligned blocks of edge x edge pixels of one face, edge = min(B, nside): in NEST order such a block is edge^2
// consecutive rows (the Morton code of (ix, iy) under the block's own), and the RING index of each of its pixels follows from
// (face, ix, iy) by the arithmetic of the HEALPix projection (Gorski et al. 2005: ring jr = jrll[face] nside - ix - iy - 1, position
// in the ring jp from ix - iy).  to_nest reads the RING rows and writes the NEST run, the other direction reads the NEST run and writes
// the RING rows: the device never inverts the RING numbering, so there is no table and no square root.  Inside a face a ring is an
// anti-diagonal ix + iy = const, and along it (ix + 1, iy - 1) is the next RING index (but for the phi = 2 pi wrap on the faces that
// straddle it): a block meets 2 edge - 1 rings in runs of 1 .. edge .. 1 consecutive RING rows.
//
// Rows narrower than a cache line (F < 32 floats): healpix_ring_to_nest_kernel / healpix_nest_to_ring_kernel turn the block through
// an LDS image in NEST order.  The RING side walks the block diagonal by diagonal, consecutive lanes on consecutive floats of a run
// (diagonals d and d + edge together hold edge pixels, which makes the walk a plain edge x edge loop); the NEST side is one linear
// copy of the image, 16 bytes per lane where the map is aligned.  B is the largest power of two with B^2 F <= 4096 floats (64, 32,
// 16, 8 for F = 1, 2-4, 5-16, 17-31): a 16 KiB image, and runs that average B / 2 rows.
// Wide rows (F >= 32): healpix_reorder_rows_kernel copies row by row, F / VEC lanes per row, blocks of 8 x 8 pixels, no LDS: a row
// is a cache line or more on both sides already.
// A run ends inside a cache line that the neighbouring block's run continues; workgroups are dealt to the XCDs in contiguous ranges
// of blocks (xcd_remap), so that the two halves of such a line meet in one L2.
//
// VEC (dsphere_mapops.h: vec_width) is the width of the accesses that address single rows; an odd F or a misaligned view runs scalar.
// Grid: x = the blocks of one map (at most 12 (8192 / 8)^2 = 12,582,912), y = min(N, 65535) maps, further maps on further trips.
#include <algorithm>

#include "dsphere_mapops.h"

namespace dsph {

constexpr int RO_THREADS = 256;
constexpr int RO_LDS_FLOATS = 4096;   // the LDS image of a block
constexpr int RO_BATCH = 4;           // independent accesses a lane keeps in flight
constexpr int RO_WIDE_F = 32;         // rows of a cache line (128 bytes) or more are copied row by row
constexpr int RO_WIDE_LGE = 3;        // ... in blocks of 8 x 8 pixels
constexpr int RO_MAX_NSIDE = 8192;    // 12 nside^2 - 1 fits int32 up to here
constexpr int RO_MAX_GRID_Y = 65535;

// even bits of a Morton code below 2^26 (nside <= 8192) packed into the low half
__host__ __device__ __forceinline__ uint32_t ro_compress(uint32_t v) {
  v &= 0x55555555u;
  v = (v | (v >> 1)) & 0x33333333u;
  v = (v | (v >> 2)) & 0x0f0f0f0fu;
  v = (v | (v >> 4)) & 0x00ff00ffu;
  v = (v | (v >> 8)) & 0x0000ffffu;
  return v;
}
__host__ __device__ __forceinline__ uint32_t ro_spread(uint32_t v) {  // bit i -> bit 2 i, v < 2^16
  v = (v | (v << 8)) & 0x00ff00ffu;
  v = (v | (v << 4)) & 0x0f0f0f0fu;
  v = (v | (v << 2)) & 0x33333333u;
  v = (v | (v << 1)) & 0x55555555u;
  return v;
}

// RING index of pixel (ix, iy) of `face` (healpix.py: nest2ring, the same arithmetic).  nside <= 8192: every term fits int32.
__host__ __device__ __forceinline__ int32_t ro_ring_index(int32_t nside, int32_t face, int32_t ix, int32_t iy) {
  const int32_t nl4 = 4 * nside;
  const int32_t jrll = (face >> 2) + 2;
  const int32_t jpll = 2 * (face & 3) + ((face >> 2) == 1 ? 0 : 1);
  const int32_t jr = jrll * nside - ix - iy - 1;
  int32_t nr, before, kshift;
  if (jr < nside) {  // north cap: ring jr has 4 jr pixels
    nr = jr; before = 2 * nr * (nr - 1); kshift = 0;
  } else if (jr > 3 * nside) {  // south cap
    nr = nl4 - jr; before = 12 * nside * nside - 2 * (nr + 1) * nr; kshift = 0;
  } else {  // belt: 4 nside pixels a ring, every other ring shifted by half a pixel
    nr = nside; before = 2 * nside * (nside - 1) + (jr - nside) * nl4; kshift = (jr - nside) & 1;
  }
  int32_t jp = (jpll * nr + ix - iy + 1 + kshift) >> 1;  // (the sum is even)
  if (jp > nl4) jp -= nl4;
  if (jp < 1) jp += nl4;
  return before + jp - 1;
}

// One block of (1 << lge)^2 pixels per workgroup and map, through an LDS image in NEST order.  VEC: floats per access on the RING
// side (F % VEC == 0, maps aligned to 4 VEC bytes); nest4: the NEST run moves as float4 (maps 16-byte aligned, run a multiple of 4).
// BATCH: a lane computes the addresses of RO_BATCH items, issues their loads and then their stores, instead of one item at a time
// (which waits for each load before the next is issued).  Measured in one process at nside 1024, batched against plain, ms:
// F = 1 0.196 / 0.238 to NEST, 0.214 / 0.252 to RING; F = 2 0.149 / 0.158, 0.164 / 0.168; F = 4 0.305 / 0.307, 0.347 / 0.352;
// F = 16 1.196 / 1.217, 1.234 / 1.263 -- and where a block holds less than a batch per lane, F = 8 0.589 / 0.581, 0.620 / 0.624;
// F = 24 0.923 / 0.900, 1.005 / 0.925.  Hence the launcher's rule: batched where the block holds RO_THREADS RO_BATCH items.
struct ReorderBlock {  // what a workgroup knows of its block
  int face, ix0, iy0, lge, edge, Q, items, run;
  uint32_t qmagic;  // i / Q = i qmagic >> 20 for i < 4096, Q < 32
  int64_t nest0;    // the block's NEST run, in floats from the start of its map
};
__device__ __forceinline__ ReorderBlock reorder_block(int lgn, int lge, int F, int VEC) {
  ReorderBlock k;
  k.lge = lge; k.edge = 1 << lge; k.Q = F / VEC;
  k.qmagic = ((1u << 20) + (uint32_t)k.Q - 1u) / (uint32_t)k.Q;
  const int lgb = 2 * (lgn - lge);  // log2 of the blocks of a face
  const uint32_t b = xcd_remap(blockIdx.x, gridDim.x);  // neighbouring blocks, which share the cache lines their runs end in, on one L2
  k.face = (int)(b >> lgb);
  const uint32_t m = b & ((1u << lgb) - 1u);
  k.ix0 = (int)(ro_compress(m) << lge); k.iy0 = (int)(ro_compress(m >> 1) << lge);
  k.nest0 = ((int64_t)b << (2 * lge)) * F;
  k.run = (k.edge * k.edge) * F;  // <= RO_LDS_FLOATS
  k.items = (k.edge * k.edge) * k.Q;
  return k;
}
// item i of the walk along the RING side = (diagonal pair p, position t along the pair, channel group q); t <= p lies on diagonal
// p (ix + iy = p), the rest of the pair on diagonal p + edge: consecutive lanes are on consecutive floats of a RING run
__device__ __forceinline__ void reorder_item(const ReorderBlock& k, int nside, int F, int VEC, int i, int* lds, int64_t* g) {
  const int px = (int)(((uint32_t)i * k.qmagic) >> 20), q = i - px * k.Q;
  const int p = px >> k.lge, t = px & (k.edge - 1);
  const int lx = t, ly = t <= p ? p - t : k.edge + p - t;
  const int32_t ring = ro_ring_index(nside, k.face, k.ix0 + lx, k.iy0 + ly);
  *lds = (int)(ro_spread((uint32_t)lx) | (ro_spread((uint32_t)ly) << 1)) * F + q * VEC;
  *g = (int64_t)ring * F + q * VEC;
}

template <int VEC, bool BATCH>
__global__ __launch_bounds__(RO_THREADS) void healpix_ring_to_nest_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t N,
                                                                          int nside, int lgn, int lge, int F, int nest4) {
  __shared__ __attribute__((aligned(16))) float img[RO_LDS_FLOATS];
  const ReorderBlock k = reorder_block(lgn, lge, F, VEC);
  const int64_t map_floats = (int64_t)12 * nside * nside * F;
  for (int64_t n = blockIdx.y; n < N; n += gridDim.y) {
    const float* xm = x + n * map_floats;
    float* ym = y + n * map_floats + k.nest0;
    constexpr int NB = BATCH ? RO_BATCH : 1;
    for (int i0 = (int)threadIdx.x; i0 < k.items; i0 += RO_THREADS * NB) {
      int lds[NB];
      int64_t g[NB];
      float r[NB][VEC];
#pragma unroll
      for (int u = 0; u < NB; ++u) reorder_item(k, nside, F, VEC, i0 + u * RO_THREADS, &lds[u], &g[u]);
#pragma unroll
      for (int u = 0; u < NB; ++u)
        if (i0 + u * RO_THREADS < k.items) ldv<VEC>(xm + g[u], r[u]);
#pragma unroll
      for (int u = 0; u < NB; ++u)
        if (i0 + u * RO_THREADS < k.items) stv<VEC>(img + lds[u], r[u]);
    }
    __syncthreads();
    if (nest4) {
      for (int i = (int)threadIdx.x * 4; i < k.run; i += RO_THREADS * 4)
        *reinterpret_cast<float4*>(ym + i) = *reinterpret_cast<const float4*>(img + i);
    } else {
      for (int i = (int)threadIdx.x; i < k.run; i += RO_THREADS) ym[i] = img[i];
    }
    __syncthreads();  // (the image is free for the next map)
  }
}

template <int VEC, bool BATCH>
__global__ __launch_bounds__(RO_THREADS) void healpix_nest_to_ring_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t N,
                                                                          int nside, int lgn, int lge, int F, int nest4) {
  __shared__ __attribute__((aligned(16))) float img[RO_LDS_FLOATS];
  const ReorderBlock k = reorder_block(lgn, lge, F, VEC);
  const int64_t map_floats = (int64_t)12 * nside * nside * F;
  for (int64_t n = blockIdx.y; n < N; n += gridDim.y) {
    const float* xm = x + n * map_floats + k.nest0;
    float* ym = y + n * map_floats;
    if (nest4) {
      for (int i = (int)threadIdx.x * 4; i < k.run; i += RO_THREADS * 4)
        *reinterpret_cast<float4*>(img + i) = *reinterpret_cast<const float4*>(xm + i);
    } else {
      for (int i = (int)threadIdx.x; i < k.run; i += RO_THREADS) img[i] = xm[i];
    }
    __syncthreads();
    constexpr int NB = BATCH ? RO_BATCH : 1;
    for (int i0 = (int)threadIdx.x; i0 < k.items; i0 += RO_THREADS * NB) {
      int lds[NB];
      int64_t g[NB];
      float r[NB][VEC];
#pragma unroll
      for (int u = 0; u < NB; ++u) reorder_item(k, nside, F, VEC, i0 + u * RO_THREADS, &lds[u], &g[u]);
#pragma unroll
      for (int u = 0; u < NB; ++u)
        if (i0 + u * RO_THREADS < k.items) ldv<VEC>(img + lds[u], r[u]);
#pragma unroll
      for (int u = 0; u < NB; ++u)
        if (i0 + u * RO_THREADS < k.items) stv<VEC>(ym + g[u], r[u]);
    }
    __syncthreads();  // (the image is free for the next map)
  }
}

// Wide rows: F / VEC lanes copy a row; consecutive lanes walk the block's NEST run.
template <int VEC>
__global__ __launch_bounds__(RO_THREADS) void healpix_reorder_rows_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t N,
                                                                          int nside, int lgn, int lge, int F, int to_nest) {
  const int Q = F / VEC;
  const int lgb = 2 * (lgn - lge);
  const uint32_t b = xcd_remap(blockIdx.x, gridDim.x);
  const int face = (int)(b >> lgb);
  const uint32_t m = b & ((1u << lgb) - 1u);
  const int ix0 = (int)(ro_compress(m) << lge), iy0 = (int)(ro_compress(m >> 1) << lge);
  const int64_t map_floats = (int64_t)12 * nside * nside * F;
  const int64_t nest0 = ((int64_t)b << (2 * lge)) * F;
  const int items = (1 << (2 * lge)) * Q;
  for (int64_t n = blockIdx.y; n < N; n += gridDim.y) {
    const float* xm = x + n * map_floats;
    float* ym = y + n * map_floats;
    for (int i = (int)threadIdx.x; i < items; i += RO_THREADS) {
      const int k = i / Q, q = i - k * Q;  // k: the row's Morton code inside the block
      const int32_t ring = ro_ring_index(nside, face, ix0 + (int)ro_compress((uint32_t)k), iy0 + (int)ro_compress((uint32_t)k >> 1));
      const int64_t gr = (int64_t)ring * F + q * VEC, gn = nest0 + (int64_t)i * VEC;
      float r[VEC];
      ldv<VEC>(xm + (to_nest ? gr : gn), r);
      stv<VEC>(ym + (to_nest ? gn : gr), r);
    }
  }
}

// log2 of the edge of the LDS kernel's blocks: the largest power of two with edge^2 F <= RO_LDS_FLOATS, at most nside
static int reorder_lds_lge(int F, int lgn) {
  int lge = 0;
  while (lge < lgn && (int64_t)(4 << (2 * lge)) * F <= RO_LDS_FLOATS) ++lge;
  return lge;
}

}  // namespace dsph

extern "C" {

// every argument is checked here, before any launch
int dsph_healpix_reorder(const float* x, float* y, int64_t N, int32_t nside, int32_t F, int32_t to_nest, int device, void* hip_stream) {
  using namespace dsph;
  if (!x || !y) { set_error("healpix_reorder: NULL pointer (x and y are required)"); return DSPH_E_BADARG; }
  if (nside < 1 || (nside & (nside - 1)) != 0) {
    set_error("healpix_reorder: nside = %d is not a power of two >= 1", (int)nside);
    return DSPH_E_BADARG;
  }
  if (nside > RO_MAX_NSIDE) {
    set_error("healpix_reorder: nside = %d; pixel indices are int32 here, which holds up to nside %d", (int)nside, RO_MAX_NSIDE);
    return DSPH_E_UNSUPPORTED;
  }
  if (F < 1) { set_error("healpix_reorder: F = %d channels, must be at least 1", (int)F); return DSPH_E_BADARG; }
  if (N < 0) { set_error("healpix_reorder: negative batch N = %lld", (long long)N); return DSPH_E_BADARG; }
  if (to_nest != 0 && to_nest != 1) { set_error("healpix_reorder: to_nest = %d, must be 0 or 1", (int)to_nest); return DSPH_E_BADARG; }
  const int64_t npix = (int64_t)12 * nside * nside;
  const double elems = (double)N * (double)npix * (double)F;
  if (elems >= 9.0e18 / 4) { set_error("healpix_reorder: N * npix * F = %.3g elements do not fit 64-bit byte offsets", elems); return DSPH_E_UNSUPPORTED; }
  const size_t bytes = (size_t)(N * npix * (int64_t)F) * sizeof(float);
  if (ranges_overlap(x, bytes, y, bytes)) {  // (maps of no bytes overlap nothing)
    set_error("healpix_reorder: x and y overlap; a permutation of rows cannot run in place");
    return DSPH_E_BADARG;
  }
  DeviceGuard guard(device);
  if (N == 0) return DSPH_OK;
  hipStream_t stream = (hipStream_t)hip_stream;
  int lgn = 0;
  while ((1 << lgn) < nside) ++lgn;
  const int VEC = vec_width(F, ptr_bits({x, y}), true);
  const bool wide = F >= RO_WIDE_F;
  const int lge = wide ? std::min(lgn, RO_WIDE_LGE) : reorder_lds_lge(F, lgn);
  const dim3 grid((unsigned)(npix >> (2 * lge)), (unsigned)std::min<int64_t>(N, RO_MAX_GRID_Y));
  if (wide) {
    DSPH_LAUNCH_BY_VEC(VEC, healpix_reorder_rows_kernel, grid, dim3(RO_THREADS), stream, x, y, N, (int)nside, lgn, lge, (int)F, (int)to_nest);
  } else {
    const int nest4 = aligned16({x, y}) && (((int64_t)F << (2 * lge)) & 3) == 0;
    // a batch per lane where the block holds one (the measurements above)
    const bool batch = ((int64_t)(F / VEC) << (2 * lge)) >= RO_THREADS * RO_BATCH;
#define RO_LAUNCH(KERNEL, VV, BB) \
  hipLaunchKernelGGL((KERNEL<VV, BB>), grid, dim3(RO_THREADS), 0, stream, x, y, N, (int)nside, lgn, lge, (int)F, nest4)
#define RO_BY_VEC(KERNEL, BB)                  \
  switch (VEC) {                               \
    case 4: RO_LAUNCH(KERNEL, 4, BB); break;   \
    case 2: RO_LAUNCH(KERNEL, 2, BB); break;   \
    default: RO_LAUNCH(KERNEL, 1, BB); break;  \
  }
    if (to_nest) {
      if (batch) { RO_BY_VEC(healpix_ring_to_nest_kernel, true) } else { RO_BY_VEC(healpix_ring_to_nest_kernel, false) }
    } else {
      if (batch) { RO_BY_VEC(healpix_nest_to_ring_kernel, true) } else { RO_BY_VEC(healpix_nest_to_ring_kernel, false) }
    }
#undef RO_BY_VEC
#undef RO_LAUNCH
  }
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

}  // extern "C"
