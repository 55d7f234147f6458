// The RING-scheme geometry behind the neighbour searches and the interpolation (healpix_knn.hip, healpix_disc.hip, healpix_interp.hip):
// a ring's z, sin(theta) and phi step in closed form (healpix.pix2vec), NEST id <-> (ring, position) by the (face, ix, iy) arithmetic
// of healpix.nest2ring / ring2nest, the squared chord to a pixel centre, the position of a ring nearest to a phi, and the ring above
// a latitude.  Host and device; float64 throughout.
#pragma once

#include <cmath>

#include "dsphere_common.h"

namespace dsph {

__host__ __device__ __forceinline__ uint32_t knn_compress(uint32_t v) {  // even bits of a Morton code below 2^26, packed
  v &= 0x55555555u;
  v = (v | (v >> 1)) & 0x33333333u;
  v = (v | (v >> 2)) & 0x0f0f0f0fu;
  v = (v | (v >> 4)) & 0x00ff00ffu;
  v = (v | (v >> 8)) & 0x0000ffffu;
  return v;
}
__host__ __device__ __forceinline__ uint32_t knn_spread(uint32_t v) {  // bit i -> bit 2 i, v < 2^16
  v = (v | (v << 8)) & 0x00ff00ffu;
  v = (v | (v << 4)) & 0x0f0f0f0fu;
  v = (v | (v << 2)) & 0x33333333u;
  v = (v | (v << 1)) & 0x55555555u;
  return v;
}

// A ring of the RING scheme, 1 <= ring <= 4 nside - 1 counted from the north pole: its pixels per quarter nr (the ring holds
// 4 nr), whether it is shifted by half a step (belt rings only), z, sin(theta) and the phi step -- the expressions of healpix.pix2vec
struct KnnRing {
  int32_t nr, kshift;
  double z, st, step;
};
__host__ __device__ __forceinline__ KnnRing knn_ring(int32_t nside, int32_t ring) {
  KnnRing g;
  const double fact2 = 4.0 / (12.0 * (double)nside * (double)nside);
  if (ring < nside) {
    g.nr = ring; g.kshift = 0;
    g.z = 1.0 - ((double)g.nr * (double)g.nr) * fact2;
  } else if (ring > 3 * nside) {
    g.nr = 4 * nside - ring; g.kshift = 0;
    g.z = ((double)g.nr * (double)g.nr) * fact2 - 1.0;
  } else {
    g.nr = nside; g.kshift = (ring - nside) & 1;
    g.z = (double)(2 * nside - ring) * ((double)(2 * nside) * fact2);
  }
  g.st = sqrt(fmax(0.0, (1.0 - g.z) * (1.0 + g.z)));
  g.step = (M_PI / 2) / (double)g.nr;
  return g;
}
// The ring above the latitude z (healpy's ring_above): the last ring whose centres lie at or north of z, 0 above the first ring;
// the ring below it is that plus one, 4 nside below the last.  |z| <= 2/3: the belt's rings are equidistant in z; beyond: a cap
// ring's z is 1 - nr^2 / (3 nside^2)
__host__ __device__ __forceinline__ int32_t knn_ring_above(int32_t nside, double z) {
  const double az = fabs(z);
  if (az <= 2.0 / 3.0) return (int32_t)((double)nside * (2.0 - 1.5 * z));
  const int32_t iring = (int32_t)((double)nside * sqrt(3.0 * (1.0 - az)));
  return z > 0 ? iring : 4 * nside - iring - 1;
}
// RING index of a ring's first pixel (position 1), the `before` of healpix.nest2ring
__host__ __device__ __forceinline__ int32_t knn_ring_first(int32_t nside, int32_t ring) {
  if (ring < nside) return 2 * ring * (ring - 1);
  if (ring > 3 * nside) { const int32_t nr = 4 * nside - ring; return 12 * nside * nside - 2 * (nr + 1) * nr; }
  return 2 * nside * (nside - 1) + (ring - nside) * 4 * nside;
}
// healpy calls a ring "shifted" when its first centre sits half a step from phi = 0: the caps, and every other ring of the belt
__host__ __device__ __forceinline__ int32_t knn_ring_shifted(const KnnRing& g) { return 1 - g.kshift; }
__host__ __device__ __forceinline__ double knn_phi(const KnnRing& g, int32_t jp) {  // position jp = 1 .. 4 nr
  return ((double)jp - (double)(g.kshift + 1) * 0.5) * g.step;
}
// squared chord between the point (ring g, phi) and the pixel centre v: the centre of a pixel where phi is knn_phi of a position
__host__ __device__ __forceinline__ double knn_d2(const KnnRing& g, double phi, const double (&v)[3]) {
  const double dx = g.st * cos(phi) - v[0], dy = g.st * sin(phi) - v[1], dz = g.z - v[2];
  return dx * dx + dy * dy + dz * dz;
}

// NEST id -> (ring, position in the ring): healpix.nest2ring before its last line
__host__ __device__ __forceinline__ void knn_nest_to_ring(int32_t nside, int32_t lgn, int32_t pix, int32_t* ring, int32_t* jp) {
  const int32_t face = pix >> (2 * lgn);
  const uint32_t m = (uint32_t)pix & ((1u << (2 * lgn)) - 1u);
  const int32_t ix = (int32_t)knn_compress(m), iy = (int32_t)knn_compress(m >> 1);
  const int32_t nl4 = 4 * nside;
  const int32_t jrll = (face >> 2) + 2;
  const int32_t jpll = 2 * (face & 3) + ((face >> 2) == 1 ? 0 : 1);
  const int32_t jr = jrll * nside - ix - iy - 1;
  int32_t nr, kshift;
  if (jr < nside) { nr = jr; kshift = 0; }
  else if (jr > 3 * nside) { nr = nl4 - jr; kshift = 0; }
  else { nr = nside; kshift = (jr - nside) & 1; }
  int32_t p = (jpll * nr + ix - iy + 1 + kshift) >> 1;  // (the sum is even)
  if (p > nl4) p -= nl4;
  if (p < 1) p += nl4;
  *ring = jr; *jp = p;
}

// (ring, position) -> NEST id: healpix.ring2nest behind its square roots
__host__ __device__ __forceinline__ int32_t knn_ring_to_nest(int32_t nside, int32_t lgn, int32_t ring, int32_t nr, int32_t kshift,
                                                             int32_t jp) {
  int32_t face;
  if (ring < nside) {
    face = (jp - 1) / nr;
  } else if (ring > 3 * nside) {
    face = 8 + (jp - 1) / nr;
  } else {  // the belt: from the two diagonals through the pixel
    const int32_t ire = ring - nside + 1, irm = 2 * nside + 2 - ire;
    const int32_t ifm = (jp - (ire >> 1) + nside - 1) >> lgn, ifp = (jp - (irm >> 1) + nside - 1) >> lgn;
    face = ifp == ifm ? (ifp | 4) : (ifp < ifm ? ifp : ifm + 8);
  }
  const int32_t jrll = (face >> 2) + 2;
  const int32_t jpll = 2 * (face & 3) + ((face >> 2) == 1 ? 0 : 1);
  const int32_t irt = ring - jrll * nside + 1;
  int32_t ipt = 2 * jp - jpll * nr - kshift - 1;
  if (ipt >= 2 * nside) ipt -= 8 * nside;
  const int32_t ix = (ipt - irt) >> 1, iy = (-ipt - irt) >> 1;
  return (face << (2 * lgn)) + (int32_t)(knn_spread((uint32_t)ix & 0xffffu) | (knn_spread((uint32_t)iy & 0xffffu) << 1));
}

// position of ring g nearest to phi, before it is wrapped into 1 .. 4 nr (any integer serves: the guards are distances to real
// positions, so this choice decides how well the window is centred, not whether its bound holds)
__host__ __device__ __forceinline__ int32_t knn_centre(const KnnRing& g, double phi) {
  return (int32_t)floor(phi / g.step + (double)(g.kshift + 1) * 0.5 + 0.5);
}
__host__ __device__ __forceinline__ int32_t knn_wrap(int32_t j, int32_t n4) {  // into 1 .. n4
  int32_t r = (j - 1) % n4;
  if (r < 0) r += n4;
  return r + 1;
}

}  // namespace dsph
