// Spherical harmonic transforms of HEALPix maps in NEST order (healpy's map2alm / alm2map without ring weights; deepsphere/sht.py
// and healpy_layers.HealpyPowerSpectrum here).  Two stages each way, the classical split of the transform on an iso-latitude grid:
//   analysis:   F_m(ring) = sum_j x[ring, j] e^{-i m phi_j}                      (dsph_sht_ring_analysis, a direct DFT per ring)
//               a_lm      = w sum_rings lambda_lm(theta_ring) F_m(ring)          (dsph_sht_legendre_analysis), w = 4 pi / npix
//   synthesis:  F_m(ring) = sum_l a_lm lambda_lm(theta_ring)                     (dsph_sht_legendre_synthesis)
//               map[ring, j] = Re sum_m c_m F_m(ring) e^{+i m phi_j}, c_0 = 1, c_m = 2   (dsph_sht_ring_synthesis)
// Arithmetic is float64 throughout (phases, recurrence, sums); maps are read and written as float32, one float at a time, so a
// map of any 4-byte alignment is taken.  No atomics: every output element has one writer and every sum a fixed order.
//
// Layouts.  Columns c = n F + f (map x channel), C = N F of them.
//   fm   float64 [mmax + 1][4 nside - 1][C][2]   ring r = 1 .. 4 nside - 1 at index r - 1, (re, im) pairs
//   alm  float64 [N][nalm][F][2]                 healpy's packed layout, index m (2 lmax + 1 - m) / 2 + l, nalm = (lmax + 1)(lmax + 2) / 2
//
// The ring stages.  Pixels are read in place through knn_ring_to_nest (and the footprint's lut): no reordered copy.  phi_j is a
// half-integer multiple of the ring's step, phi_j = 2 pi (2 j - 1 - kshift) / (8 nr), so the phase m phi_j is reduced exactly as
// k = m (2 j - 1 - kshift) mod 8 nr before sincospi(k / (4 nr)).  An exact phase is taken every SH_RESEED terms and the terms
// between are reached by a rotation with the (equally reduced) step phase: at most SH_RESEED - 1 complex products from an exact
// value.  The DFT is direct, so m above a ring's Nyquist (any m <= mmax on a ring of 4 pixels) needs no folding.
//   analysis:  a workgroup = (ring, 256 values of m, SH_CB columns); a lane owns one m, the ring's pixels pass through LDS.
//   synthesis: a workgroup = (ring, 256 pixels, SH_CB columns); a lane owns one pixel, F_m passes through LDS.
//
// The Legendre stages.  A workgroup = (m, SH_CB columns).  It walks the northern rings and the equator (2 nside rings) in chunks of
// SH_RT; for a chunk, lane r runs the three-term recurrence of its ring in l,
//   lambda_lm = a_lm (x lambda_{l-1,m} - lambda_{l-2,m} / a_{l-1,m}),  a_lm = sqrt((4 l^2 - 1) / (l^2 - m^2)),
// SH_LT values of l at a time into an LDS tile [ring][l] (the coefficients of the SH_LT steps are computed once per tile, by SH_LT
// lanes), and the workgroup contracts the tile with F_m (analysis: over the rings) or with a_lm (synthesis: over l) on vector FMAs.
// The southern rings ride on lambda_lm(pi - theta) = (-1)^(l + m) lambda_lm(theta): analysis contracts with F(north) +- F(south),
// synthesis keeps the sums over even and odd l + m apart and stores their sum north and their difference south.
//
// Exponent range.  lambda_mm = (-1)^m sqrt((2 m + 1) / (4 pi) prod_{k <= m} (2 k - 1) / (2 k)) sin^m theta underflows float64 from
// m of a few hundred on near the poles (sin^1500 of the first ring of nside 1024 is 1e-5000), and the recurrence then grows out
// of that.  The value is therefore kept as v 2^(SH_SCALE_BITS s) with an integer s <= 0: sin^m theta by binary powering on
// (mantissa, exponent) pairs, s and v from the exponent; whenever |v| passes 2^(SH_SCALE_BITS / 2) both recurrence values are
// multiplied by 2^-SH_SCALE_BITS and s grows by one.  |lambda| < sqrt((2 l + 1) / 4 pi), so s never passes 0; while s < 0 the true
// value lies below 2^-240 = 6e-73 of a function whose largest value over the rings is of order 1, and the term is dropped.
//
// In analysis the sums of a chunk of rings are added to what the chunks before left in alm (the same lane reads what it wrote:
// a fixed order, no fence); the first chunk stores.  In synthesis a chunk of rings is finished before the next one starts.
#include <algorithm>
#include <cmath>

#include "dsphere_mapops.h"
#include "healpix_ring.h"

namespace dsph {

constexpr int SH_THREADS = 256;
constexpr int SH_CB = 8;             // columns of a workgroup
constexpr int SH_JT = 256;           // ring pixels per LDS tile (ring analysis)
constexpr int SH_MT = 128;           // values of m per LDS tile (ring synthesis)
constexpr int SH_RESEED = 16;        // an exact phase every so many terms
constexpr int SH_RT = 128;           // rings per chunk of the Legendre stages
constexpr int SH_LT = 32;            // values of l per tile (even: the parity of l + m within a tile is that of the tile's row)
constexpr int SH_LPAD = SH_LT + 1;   // row stride of the lambda tile
constexpr int SH_SCALE_BITS = 480;
constexpr int SH_MAX_NSIDE = 2048;
constexpr int SH_MAX_COL_BLOCKS = 4096;  // grid extent over the column blocks; further blocks on further trips

static_assert(SH_LT % 2 == 0 && SH_LT * SH_CB == SH_THREADS && 2 * SH_RT == SH_THREADS, "the Legendre kernels' lane maps");

// ---- ring stages ----------------------------------------------------------------------------------------------------------------

// e^{sign i pi k / (4 nr)} for an exactly reduced 0 <= k < 8 nr
__device__ __forceinline__ void sht_phase(int32_t k, int32_t nr, double sign, double* wr, double* wi) {
  double s, c;
  sincospi((double)k / (double)(4 * nr), &s, &c);
  *wr = c; *wi = sign * s;
}

__global__ __launch_bounds__(SH_THREADS) void sht_ring_analysis_kernel(const float* __restrict__ x, double* __restrict__ fm, int64_t C,
                                                                       int32_t F, int32_t nside, int32_t lgn, int32_t mmax,
                                                                       const int32_t* __restrict__ lut, int64_t M) {
  __shared__ float tile[SH_JT][SH_CB];
  __shared__ int32_t trow[SH_JT];
  const int tid = (int)threadIdx.x;
  const int32_t ring = (int32_t)blockIdx.x + 1;
  const KnnRing g = knn_ring(nside, ring);
  const int32_t n4 = 4 * g.nr, n8 = 8 * g.nr;
  const int32_t m = (int32_t)blockIdx.y * SH_THREADS + tid;
  const bool active = m <= mmax;
  const int64_t R = 4 * (int64_t)nside - 1;
  const int64_t ncb = (C + SH_CB - 1) / SH_CB;
  double sr, si;  // the step between neighbouring pixels: phase 2 m
  sht_phase((int32_t)((2 * (int64_t)m) % n8), g.nr, -1.0, &sr, &si);
  for (int64_t cb = blockIdx.z; cb < ncb; cb += gridDim.z) {
    const int64_t c0 = cb * SH_CB;
    double re[SH_CB], im[SH_CB];
#pragma unroll
    for (int cc = 0; cc < SH_CB; ++cc) { re[cc] = 0.0; im[cc] = 0.0; }
    for (int32_t j0 = 0; j0 < n4; j0 += SH_JT) {
      const int nj = n4 - j0 < SH_JT ? n4 - j0 : SH_JT;
      __syncthreads();  // the tile before has been read
      if (tid < nj) {
        const int32_t nest = knn_ring_to_nest(nside, lgn, ring, g.nr, g.kshift, j0 + tid + 1);
        const int32_t row = lut ? lut[nest] : nest;
        trow[tid] = (row >= 0 && row < M) ? row : -1;  // (outside the footprint: zero)
      }
      __syncthreads();
      for (int idx = tid; idx < nj * SH_CB; idx += SH_THREADS) {
        const int jl = idx / SH_CB, cc = idx % SH_CB;
        const int64_t c = c0 + cc;
        float v = 0.0f;
        if (c < C && trow[jl] >= 0) {
          const int64_t n = c / F, f = c - n * F;
          v = x[(n * M + trow[jl]) * F + f];
        }
        tile[jl][cc] = v;
      }
      __syncthreads();
      if (active) {
        for (int jb = 0; jb < nj; jb += SH_RESEED) {
          double wr, wi;
          const int64_t q = 2 * (int64_t)(j0 + jb + 1) - 1 - g.kshift;
          sht_phase((int32_t)(((int64_t)m * q) % n8), g.nr, -1.0, &wr, &wi);
          const int ne = nj - jb < SH_RESEED ? nj - jb : SH_RESEED;
          for (int u = 0; u < ne; ++u) {
#pragma unroll
            for (int cc = 0; cc < SH_CB; ++cc) {
              const double v = (double)tile[jb + u][cc];
              re[cc] = fma(v, wr, re[cc]);
              im[cc] = fma(v, wi, im[cc]);
            }
            const double t = wr * sr - wi * si;
            wi = wr * si + wi * sr;
            wr = t;
          }
        }
      }
    }
    if (active) {
      double* out = fm + (((int64_t)m * R + (ring - 1)) * C + c0) * 2;
#pragma unroll
      for (int cc = 0; cc < SH_CB; ++cc)
        if (c0 + cc < C) { out[2 * cc] = re[cc]; out[2 * cc + 1] = im[cc]; }
    }
  }
}

__global__ __launch_bounds__(SH_THREADS) void sht_ring_synthesis_kernel(const double* __restrict__ fm, float* __restrict__ y, int64_t C,
                                                                        int32_t F, int32_t nside, int32_t lgn, int32_t mmax,
                                                                        const int32_t* __restrict__ lut, int64_t M) {
  __shared__ double ft[SH_MT][SH_CB][2];
  const int tid = (int)threadIdx.x;
  const int32_t ring = (int32_t)blockIdx.x + 1;
  const KnnRing g = knn_ring(nside, ring);
  const int32_t n4 = 4 * g.nr, n8 = 8 * g.nr;
  if ((int32_t)blockIdx.y * SH_THREADS >= n4) return;  // (the whole workgroup: a shorter ring)
  const int32_t jp = (int32_t)blockIdx.y * SH_THREADS + tid + 1;
  int32_t row = -1;
  if (jp <= n4) {
    const int32_t nest = knn_ring_to_nest(nside, lgn, ring, g.nr, g.kshift, jp);
    row = lut ? lut[nest] : nest;
    if (row < 0 || row >= M) row = -1;  // (outside the footprint: not written)
  }
  const int64_t q = 2 * (int64_t)jp - 1 - g.kshift;
  const int64_t R = 4 * (int64_t)nside - 1;
  const int64_t ncb = (C + SH_CB - 1) / SH_CB;
  double sr, si;  // the step between neighbouring m: phase q
  sht_phase((int32_t)(q % n8), g.nr, 1.0, &sr, &si);
  for (int64_t cb = blockIdx.z; cb < ncb; cb += gridDim.z) {
    const int64_t c0 = cb * SH_CB;
    double acc[SH_CB];
#pragma unroll
    for (int cc = 0; cc < SH_CB; ++cc) acc[cc] = 0.0;
    for (int32_t m0 = 0; m0 <= mmax; m0 += SH_MT) {
      const int nm = mmax + 1 - m0 < SH_MT ? mmax + 1 - m0 : SH_MT;
      __syncthreads();  // the tile before has been read
      for (int idx = tid; idx < nm * SH_CB; idx += SH_THREADS) {
        const int ml = idx / SH_CB, cc = idx % SH_CB;
        const int64_t c = c0 + cc;
        double a = 0.0, b = 0.0;
        if (c < C) {
          const double* in = fm + (((int64_t)(m0 + ml) * R + (ring - 1)) * C + c) * 2;
          const double mult = m0 + ml == 0 ? 1.0 : 2.0;  // m = 0 counts once, m > 0 as 2 Re
          a = mult * in[0]; b = mult * in[1];
        }
        ft[ml][cc][0] = a; ft[ml][cc][1] = b;
      }
      __syncthreads();
      if (row >= 0) {
        for (int mb = 0; mb < nm; mb += SH_RESEED) {
          double wr, wi;
          sht_phase((int32_t)(((int64_t)(m0 + mb) * q) % n8), g.nr, 1.0, &wr, &wi);
          const int ne = nm - mb < SH_RESEED ? nm - mb : SH_RESEED;
          for (int u = 0; u < ne; ++u) {
#pragma unroll
            for (int cc = 0; cc < SH_CB; ++cc) acc[cc] = fma(ft[mb + u][cc][0], wr, fma(-ft[mb + u][cc][1], wi, acc[cc]));
            const double t = wr * sr - wi * si;
            wi = wr * si + wi * sr;
            wr = t;
          }
        }
      }
    }
    if (row >= 0) {
#pragma unroll
      for (int cc = 0; cc < SH_CB; ++cc) {
        const int64_t c = c0 + cc;
        if (c < C) {
          const int64_t n = c / F, f = c - n * F;
          y[(n * M + row) * F + f] = (float)acc[cc];
        }
      }
    }
  }
}

// ---- Legendre stages ------------------------------------------------------------------------------------------------------------

// prod_{k = 1 .. m} (2 k - 1) / (2 k) >= 1 / sqrt(pi m + 1): plain float64; a slice per lane, then lane 0 in ascending order
__device__ __forceinline__ double sht_mfac(int32_t m, double* red, int tid) {
  double p = 1.0;
  for (int32_t k = tid + 1; k <= m; k += SH_THREADS) p *= (double)(2 * k - 1) / (double)(2 * k);
  red[tid] = p;
  __syncthreads();
  if (tid == 0) {
    for (int t = 1; t < SH_THREADS; ++t) p *= red[t];
    red[0] = p;
  }
  __syncthreads();
  p = red[0];
  __syncthreads();
  return p;
}

// The recurrence of one ring: true value = v1 2^(SH_SCALE_BITS s) (v2: the value one l back, on the same scale)
struct ShtRec {
  double x, v1, v2;
  int32_t s;
};
// lambda_mm at the ring (x = cos theta, st = sin theta > 0); pref = (-1)^m sqrt((2 m + 1) / (4 pi) prod) in plain float64
__device__ __forceinline__ ShtRec sht_rec_start(double x, double st, int32_t m, double pref) {
  int be;
  double bm = frexp(st, &be);  // st = bm 2^be, bm in [0.5, 1)
  double rm = 1.0;
  int64_t bexp = be, rexp = 0;
  for (int32_t bits = m; bits; bits >>= 1) {  // st^m by squaring, mantissa and exponent apart
    int e;
    if (bits & 1) {
      rm = frexp(rm * bm, &e);
      rexp += bexp + e;
    }
    bm = frexp(bm * bm, &e);
    bexp = 2 * bexp + e;
  }
  int e;
  const double f = frexp(pref * rm, &e);  // |f| in [0.5, 1)
  const int64_t T = rexp + e;             // lambda_mm = f 2^T, T <= 0 up to the rounding of a value below 1
  int32_t s = T < 0 ? -(int32_t)((-T) / SH_SCALE_BITS) : 0;
  ShtRec r;
  r.x = x; r.s = s; r.v2 = 0.0;
  r.v1 = ldexp(f, (int)(T - (int64_t)SH_SCALE_BITS * s));  // exponent in (-SH_SCALE_BITS, 0], or T itself when T > 0
  return r;
}
// the coefficients of the step to l (l > m): A = a_lm, B = a_lm / a_{l-1,m} (0 at l = m + 1: there is no lambda_{m-1,m})
__device__ __forceinline__ void sht_coef(int32_t l, int32_t m, double* A, double* B) {
  const double dl = (double)l, dm = (double)m;
  const double a = sqrt((4.0 * dl * dl - 1.0) / ((dl - dm) * (dl + dm)));
  *A = a;
  if (l == m + 1) { *B = 0.0; return; }
  const double l1 = dl - 1.0;
  *B = a / sqrt((4.0 * l1 * l1 - 1.0) / ((l1 - dm) * (l1 + dm)));
}
// nl values of l from l0 on into lam[0 .. nl) (l0 = m: the first is lambda_mm itself); a value on a negative scale is stored as 0
__device__ __forceinline__ void sht_rec_tile(ShtRec& r, int32_t l0, int32_t m, int nl, const double* sA, const double* sB, double* lam) {
  const double big = ldexp(1.0, SH_SCALE_BITS / 2), down = ldexp(1.0, -SH_SCALE_BITS);
  for (int i = 0; i < nl; ++i) {
    if (l0 + i > m) {
      const double vn = sA[i] * r.x * r.v1 - sB[i] * r.v2;
      r.v2 = r.v1; r.v1 = vn;
      if (fabs(vn) > big) { r.v1 *= down; r.v2 *= down; r.s += 1; }
    }
    lam[i] = r.s == 0 ? r.v1 : 0.0;
  }
}

__device__ __forceinline__ int64_t sht_alm_index(int32_t lmax, int32_t l, int32_t m) {
  return ((int64_t)m * (2 * (int64_t)lmax + 1 - m)) / 2 + l;
}

__global__ __launch_bounds__(SH_THREADS) void sht_legendre_analysis_kernel(const double* __restrict__ fm, double* alm, int64_t C, int32_t F,
                                                                           int32_t nside, int32_t lmax, double w) {
  __shared__ double lam[SH_RT][SH_LPAD];
  __shared__ double ftile[SH_RT][2][SH_CB][2];  // [ring][north + south, north - south][column][re, im], times w
  __shared__ double sA[SH_LT], sB[SH_LT];
  __shared__ double red[SH_THREADS];
  const int tid = (int)threadIdx.x;
  const int32_t m = (int32_t)blockIdx.x;
  const int64_t R = 4 * (int64_t)nside - 1, nalm = ((int64_t)lmax + 1) * ((int64_t)lmax + 2) / 2;
  const int32_t nrn = 2 * nside;  // the northern rings and the equator
  const int64_t ncb = (C + SH_CB - 1) / SH_CB;
  const double pref = ((m & 1) ? -1.0 : 1.0) * sqrt((double)(2 * m + 1) / (4.0 * M_PI) * sht_mfac(m, red, tid));
  const int ll = tid / SH_CB, cc = tid % SH_CB;  // the lane's element of a tile of sums
  for (int64_t cb = blockIdx.y; cb < ncb; cb += gridDim.y) {
    const int64_t c0 = cb * SH_CB, c = c0 + cc;
    const int64_t n = c / F, f = c - n * F;
    for (int32_t r0 = 0; r0 < nrn; r0 += SH_RT) {
      __syncthreads();  // the chunk before has been read
      for (int idx = tid; idx < SH_RT * SH_CB; idx += SH_THREADS) {
        const int rl = idx / SH_CB, ci = idx % SH_CB;
        const int32_t ring = r0 + rl + 1;
        double nr_ = 0.0, ni_ = 0.0, sr_ = 0.0, si_ = 0.0;
        if (ring <= nrn && c0 + ci < C) {
          const double* pn = fm + (((int64_t)m * R + (ring - 1)) * C + c0 + ci) * 2;
          nr_ = pn[0]; ni_ = pn[1];
          if (ring < nrn) {
            const double* ps = fm + (((int64_t)m * R + (4 * nside - ring - 1)) * C + c0 + ci) * 2;
            sr_ = ps[0]; si_ = ps[1];
          }
        }
        ftile[rl][0][ci][0] = w * (nr_ + sr_); ftile[rl][0][ci][1] = w * (ni_ + si_);
        ftile[rl][1][ci][0] = w * (nr_ - sr_); ftile[rl][1][ci][1] = w * (ni_ - si_);
      }
      ShtRec rec;
      const bool gen = tid < SH_RT && r0 + tid + 1 <= nrn;
      if (gen) {
        const KnnRing g = knn_ring(nside, r0 + tid + 1);
        rec = sht_rec_start(g.z, g.st, m, pref);
      }
      for (int32_t l0 = m; l0 <= lmax; l0 += SH_LT) {
        const int nl = lmax + 1 - l0 < SH_LT ? lmax + 1 - l0 : SH_LT;
        __syncthreads();  // the tile before has been read (the first time: ftile is complete)
        if (tid < nl && l0 + tid > m) sht_coef(l0 + tid, m, &sA[tid], &sB[tid]);
        __syncthreads();
        if (tid < SH_RT) {
          if (gen) {
            sht_rec_tile(rec, l0, m, nl, sA, sB, lam[tid]);
          } else {
            for (int i = 0; i < nl; ++i) lam[tid][i] = 0.0;
          }
        }
        __syncthreads();
        if (ll < nl && c < C) {
          const int par = ll & 1;  // the parity of l + m: l0 - m is a multiple of SH_LT
          double ar = 0.0, ai = 0.0;
          for (int rl = 0; rl < SH_RT; ++rl) {
            const double lv = lam[rl][ll];
            ar = fma(lv, ftile[rl][par][cc][0], ar);
            ai = fma(lv, ftile[rl][par][cc][1], ai);
          }
          double* out = alm + ((n * nalm + sht_alm_index(lmax, l0 + ll, m)) * F + f) * 2;
          if (r0 > 0) { ar += out[0]; ai += out[1]; }  // (this lane wrote them, a chunk of rings ago)
          out[0] = ar; out[1] = ai;
        }
      }
    }
  }
}

__global__ __launch_bounds__(SH_THREADS) void sht_legendre_synthesis_kernel(const double* __restrict__ alm, double* __restrict__ fm, int64_t C,
                                                                            int32_t F, int32_t nside, int32_t lmax) {
  __shared__ double lam[SH_RT][SH_LPAD];
  __shared__ double atile[SH_LT][SH_CB][2];
  __shared__ double sA[SH_LT], sB[SH_LT];
  __shared__ double red[SH_THREADS];
  const int tid = (int)threadIdx.x;
  const int32_t m = (int32_t)blockIdx.x;
  const int64_t R = 4 * (int64_t)nside - 1, nalm = ((int64_t)lmax + 1) * ((int64_t)lmax + 2) / 2;
  const int32_t nrn = 2 * nside;
  const int64_t ncb = (C + SH_CB - 1) / SH_CB;
  const double pref = ((m & 1) ? -1.0 : 1.0) * sqrt((double)(2 * m + 1) / (4.0 * M_PI) * sht_mfac(m, red, tid));
  const int rl = tid / 2, h = tid % 2;  // the lane's ring of a chunk and its half of the columns
  constexpr int HC = SH_CB / 2;
  for (int64_t cb = blockIdx.y; cb < ncb; cb += gridDim.y) {
    const int64_t c0 = cb * SH_CB;
    for (int32_t r0 = 0; r0 < nrn; r0 += SH_RT) {
      double acc[2][HC][2];  // [parity of l + m][column][re, im]
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int j = 0; j < HC; ++j) { acc[p][j][0] = 0.0; acc[p][j][1] = 0.0; }
      ShtRec rec;
      const bool gen = tid < SH_RT && r0 + tid + 1 <= nrn;
      if (gen) {
        const KnnRing g = knn_ring(nside, r0 + tid + 1);
        rec = sht_rec_start(g.z, g.st, m, pref);
      }
      for (int32_t l0 = m; l0 <= lmax; l0 += SH_LT) {
        const int nl = lmax + 1 - l0 < SH_LT ? lmax + 1 - l0 : SH_LT;
        __syncthreads();  // the tiles before have been read
        if (tid < nl && l0 + tid > m) sht_coef(l0 + tid, m, &sA[tid], &sB[tid]);
        {
          const int li = tid / SH_CB, ci = tid % SH_CB;  // SH_LT * SH_CB == SH_THREADS: an element of the tile per lane
          const int64_t c = c0 + ci;
          double a = 0.0, b = 0.0;
          if (li < nl && c < C) {
            const int64_t n = c / F, f = c - n * F;
            const double* in = alm + ((n * nalm + sht_alm_index(lmax, l0 + li, m)) * F + f) * 2;
            a = in[0]; b = in[1];
          }
          atile[li][ci][0] = a; atile[li][ci][1] = b;
        }
        __syncthreads();
        if (tid < SH_RT) {
          if (gen) {
            sht_rec_tile(rec, l0, m, nl, sA, sB, lam[tid]);
          } else {
            for (int i = 0; i < nl; ++i) lam[tid][i] = 0.0;
          }
        }
        __syncthreads();
        for (int i = 0; i < nl; ++i) {
          const double lv = lam[rl][i];
          const int p = i & 1;
#pragma unroll
          for (int j = 0; j < HC; ++j) {
            if (p == 0) {
              acc[0][j][0] = fma(lv, atile[i][h * HC + j][0], acc[0][j][0]);
              acc[0][j][1] = fma(lv, atile[i][h * HC + j][1], acc[0][j][1]);
            } else {
              acc[1][j][0] = fma(lv, atile[i][h * HC + j][0], acc[1][j][0]);
              acc[1][j][1] = fma(lv, atile[i][h * HC + j][1], acc[1][j][1]);
            }
          }
        }
      }
      const int32_t ring = r0 + rl + 1;
      if (ring <= nrn) {
#pragma unroll
        for (int j = 0; j < HC; ++j) {
          const int64_t c = c0 + h * HC + j;
          if (c < C) {
            double* pn = fm + (((int64_t)m * R + (ring - 1)) * C + c) * 2;
            pn[0] = acc[0][j][0] + acc[1][j][0]; pn[1] = acc[0][j][1] + acc[1][j][1];
            if (ring < nrn) {
              double* ps = fm + (((int64_t)m * R + (4 * nside - ring - 1)) * C + c) * 2;
              ps[0] = acc[0][j][0] - acc[1][j][0]; ps[1] = acc[0][j][1] - acc[1][j][1];
            }
          }
        }
      }
    }
  }
}

// ---- argument checks ------------------------------------------------------------------------------------------------------------

static int sht_shape_ok(const char* who, int64_t N, int32_t nside, int32_t F, int32_t lmax, const char* lname) {
  if (nside < 1 || (nside & (nside - 1)) != 0) {
    set_error("%s: nside = %d is not a power of two >= 1", who, (int)nside);
    return DSPH_E_BADARG;
  }
  if (nside > SH_MAX_NSIDE) {
    set_error("%s: nside = %d; the transform takes nside up to %d", who, (int)nside, SH_MAX_NSIDE);
    return DSPH_E_UNSUPPORTED;
  }
  if (lmax < 0 || lmax > 4 * nside - 1) {
    set_error("%s: %s = %d outside [0, 4 nside - 1 = %d]", who, lname, (int)lmax, (int)(4 * nside - 1));
    return DSPH_E_BADARG;
  }
  if (F < 1) { set_error("%s: F = %d channels, must be at least 1", who, (int)F); return DSPH_E_BADARG; }
  if (N < 0) { set_error("%s: negative batch N = %lld", who, (long long)N); return DSPH_E_BADARG; }
  return DSPH_OK;
}

static int sht_set_ok(const char* who, int32_t nside, const int32_t* lut, const int64_t* indices, int64_t M) {
  const int64_t npix = (int64_t)12 * nside * nside;
  if ((indices == nullptr) != (lut == nullptr)) {
    set_error("%s: indices and lut come together (both NULL: the full sky)", who);
    return DSPH_E_BADARG;
  }
  if (!indices && M != npix) {
    set_error("%s: M = %lld rows without indices, the full sky of nside %d has %lld", who, (long long)M, (int)nside, (long long)npix);
    return DSPH_E_BADARG;
  }
  if (M < 0 || M > npix) {
    set_error("%s: M = %lld rows outside [0, 12 nside^2 = %lld]", who, (long long)M, (long long)npix);
    return DSPH_E_BADARG;
  }
  return DSPH_OK;
}

// bytes of the three arrays; 0 with an error set when they do not fit 64-bit offsets
static bool sht_sizes(const char* who, int64_t N, int32_t nside, int32_t F, int32_t lmax, int64_t M, size_t* map_bytes, size_t* fm_bytes,
                      size_t* alm_bytes) {
  const double C = (double)N * (double)F, R = 4.0 * nside - 1.0, nalm = 0.5 * (lmax + 1.0) * (lmax + 2.0);
  if (C * std::max(std::max((double)M, (lmax + 1.0) * R * 2.0), nalm * 2.0) >= 9.0e18 / 8) {
    set_error("%s: N * F = %.3g columns do not fit 64-bit byte offsets", who, C);
    return false;
  }
  const int64_t Ci = N * (int64_t)F;
  *map_bytes = (size_t)(Ci * M) * sizeof(float);
  *fm_bytes = (size_t)(Ci * (lmax + 1) * (4 * (int64_t)nside - 1) * 2) * sizeof(double);
  *alm_bytes = (size_t)(Ci * (((int64_t)lmax + 1) * ((int64_t)lmax + 2) / 2) * 2) * sizeof(double);
  return true;
}

static int sht_lg(int32_t nside) {
  int lgn = 0;
  while ((1 << lgn) < nside) ++lgn;
  return lgn;
}

static unsigned sht_col_grid(int64_t C) { return (unsigned)std::min<int64_t>((C + SH_CB - 1) / SH_CB, SH_MAX_COL_BLOCKS); }

}  // namespace dsph

extern "C" {

// every argument is checked here, before any launch
int dsph_sht_ring_analysis(const float* x, double* fm, int64_t N, int32_t nside, int32_t F, int32_t mmax, const int32_t* lut,
                           const int64_t* indices, int64_t M, int device, void* hip_stream) {
  using namespace dsph;
  const char* who = "sht_ring_analysis";
  if (!x || !fm) { set_error("%s: NULL pointer (x and fm are required)", who); return DSPH_E_BADARG; }
  int rc = sht_shape_ok(who, N, nside, F, mmax, "mmax");
  if (rc == DSPH_OK) rc = sht_set_ok(who, nside, lut, indices, M);
  if (rc != DSPH_OK) return rc;
  if (reinterpret_cast<uintptr_t>(fm) & 7) { set_error("%s: fm is not 8-byte aligned", who); return DSPH_E_BADARG; }
  size_t xb, fb, ab;
  if (!sht_sizes(who, N, nside, F, mmax, M, &xb, &fb, &ab)) return DSPH_E_UNSUPPORTED;
  if (ranges_overlap(x, xb, fm, fb)) { set_error("%s: x and fm overlap", who); return DSPH_E_BADARG; }
  DeviceGuard guard(device);
  if (!select_device(who, device, guard)) return DSPH_E_HIP;
  if (N == 0) return DSPH_OK;
  const int64_t C = N * (int64_t)F;
  const dim3 grid((unsigned)(4 * nside - 1), (unsigned)((mmax + SH_THREADS) / SH_THREADS), sht_col_grid(C));
  hipLaunchKernelGGL(sht_ring_analysis_kernel, grid, dim3(SH_THREADS), 0, (hipStream_t)hip_stream, x, fm, C, F, nside, (int32_t)sht_lg(nside),
                     mmax, lut, M);
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

int dsph_sht_ring_synthesis(const double* fm, float* y, int64_t N, int32_t nside, int32_t F, int32_t mmax, const int32_t* lut,
                            const int64_t* indices, int64_t M, int device, void* hip_stream) {
  using namespace dsph;
  const char* who = "sht_ring_synthesis";
  if (!fm || !y) { set_error("%s: NULL pointer (fm and y are required)", who); return DSPH_E_BADARG; }
  int rc = sht_shape_ok(who, N, nside, F, mmax, "mmax");
  if (rc == DSPH_OK) rc = sht_set_ok(who, nside, lut, indices, M);
  if (rc != DSPH_OK) return rc;
  if (reinterpret_cast<uintptr_t>(fm) & 7) { set_error("%s: fm is not 8-byte aligned", who); return DSPH_E_BADARG; }
  size_t yb, fb, ab;
  if (!sht_sizes(who, N, nside, F, mmax, M, &yb, &fb, &ab)) return DSPH_E_UNSUPPORTED;
  if (ranges_overlap(y, yb, fm, fb)) { set_error("%s: fm and y overlap", who); return DSPH_E_BADARG; }
  DeviceGuard guard(device);
  if (!select_device(who, device, guard)) return DSPH_E_HIP;
  if (N == 0 || M == 0) return DSPH_OK;
  const int64_t C = N * (int64_t)F;
  const dim3 grid((unsigned)(4 * nside - 1), (unsigned)((4 * nside + SH_THREADS - 1) / SH_THREADS), sht_col_grid(C));
  hipLaunchKernelGGL(sht_ring_synthesis_kernel, grid, dim3(SH_THREADS), 0, (hipStream_t)hip_stream, fm, y, C, F, nside,
                     (int32_t)sht_lg(nside), mmax, lut, M);
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

int dsph_sht_legendre_analysis(const double* fm, double* alm, int64_t N, int32_t nside, int32_t F, int32_t lmax, int device,
                               void* hip_stream) {
  using namespace dsph;
  const char* who = "sht_legendre_analysis";
  if (!fm || !alm) { set_error("%s: NULL pointer (fm and alm are required)", who); return DSPH_E_BADARG; }
  const int rc = sht_shape_ok(who, N, nside, F, lmax, "lmax");
  if (rc != DSPH_OK) return rc;
  if ((reinterpret_cast<uintptr_t>(fm) | reinterpret_cast<uintptr_t>(alm)) & 7) {
    set_error("%s: fm or alm is not 8-byte aligned", who);
    return DSPH_E_BADARG;
  }
  size_t xb, fb, ab;
  if (!sht_sizes(who, N, nside, F, lmax, 0, &xb, &fb, &ab)) return DSPH_E_UNSUPPORTED;
  if (ranges_overlap(fm, fb, alm, ab)) { set_error("%s: fm and alm overlap", who); return DSPH_E_BADARG; }
  DeviceGuard guard(device);
  if (!select_device(who, device, guard)) return DSPH_E_HIP;
  if (N == 0) return DSPH_OK;
  const int64_t C = N * (int64_t)F;
  const double w = 4.0 * M_PI / (12.0 * (double)nside * (double)nside);
  hipLaunchKernelGGL(sht_legendre_analysis_kernel, dim3((unsigned)(lmax + 1), sht_col_grid(C)), dim3(SH_THREADS), 0, (hipStream_t)hip_stream,
                     fm, alm, C, F, nside, lmax, w);
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

int dsph_sht_legendre_synthesis(const double* alm, double* fm, int64_t N, int32_t nside, int32_t F, int32_t lmax, int device,
                                void* hip_stream) {
  using namespace dsph;
  const char* who = "sht_legendre_synthesis";
  if (!fm || !alm) { set_error("%s: NULL pointer (alm and fm are required)", who); return DSPH_E_BADARG; }
  const int rc = sht_shape_ok(who, N, nside, F, lmax, "lmax");
  if (rc != DSPH_OK) return rc;
  if ((reinterpret_cast<uintptr_t>(fm) | reinterpret_cast<uintptr_t>(alm)) & 7) {
    set_error("%s: alm or fm is not 8-byte aligned", who);
    return DSPH_E_BADARG;
  }
  size_t xb, fb, ab;
  if (!sht_sizes(who, N, nside, F, lmax, 0, &xb, &fb, &ab)) return DSPH_E_UNSUPPORTED;
  if (ranges_overlap(fm, fb, alm, ab)) { set_error("%s: alm and fm overlap", who); return DSPH_E_BADARG; }
  DeviceGuard guard(device);
  if (!select_device(who, device, guard)) return DSPH_E_HIP;
  if (N == 0) return DSPH_OK;
  const int64_t C = N * (int64_t)F;
  hipLaunchKernelGGL(sht_legendre_synthesis_kernel, dim3((unsigned)(lmax + 1), sht_col_grid(C)), dim3(SH_THREADS), 0,
                     (hipStream_t)hip_stream, alm, fm, C, F, nside, lmax);
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

}  // extern "C"
