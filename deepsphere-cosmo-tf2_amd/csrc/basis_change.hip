// A change of polynomial basis on a layer's weights: the small linear map that turns a Bernstein layer into a Chebyshev one.
//     w_out[f*Kp + j, o] = sum_i c(i,j) * w[f*Kp + i, o],   c(i,j) = coeff[i*Kp + j]  (transpose = 0)  |  coeff[j*Kp + i]  (transpose = 1)
// With row i of coeff the Chebyshev coefficients of the layer's i-th polynomial, sum_i B_i(L~) x W_i = sum_j T_j(L~) x W'_j for
// W' = basis_change(W, transpose = 0): the layer runs every fused, strip and tile kernel of the Chebyshev path on W', and the
// weight gradient those kernels return (in the T_j basis) goes back through the same map with transpose = 1.  Replaces the
// K (K + 1) sparse products of the reference's Bernstein.call (gnn_layers.py:543-554) by nothing on the map side.
//
// The work is tiny (Fin * Kp * Fout outputs of Kp multiply-adds; 64 -> 64 at Kp = 6: 24,576 outputs), so the kernel is the plain
// one: a thread owns VEC neighbouring output columns of one output row, walks i = 0 .. Kp - 1 in that order with one fp32 fma
// per step (deterministic; the tests' bound is derived from this order), the Kp rows of w it reads are Kp coalesced row
// segments, its Kp coefficients one column (or row) of a table of at most 16 KB that stays in the caches.  One writer per
// element, no atomics, no shared memory.  Every element offset is 64-bit.
#include "dsphere_mapops.h"

namespace dsph {

namespace {

// total = Fin * Kp * (Fout / VEC) threads do work; thread t: column vector q = t % nv of output row r = t / nv = f * Kp + j
template <int VEC>
__global__ __launch_bounds__(256) void basis_change_kernel(const float* __restrict__ w, const float* __restrict__ coeff,
                                                           float* __restrict__ w_out, int Fout, int Kp, int transpose, int64_t total) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int nv = Fout / VEC;
  const int64_t r = t / nv;
  const int q = (int)(t - r * nv);
  const int j = (int)(r % Kp);
  const float* __restrict__ wf = w + (r - j) * Fout + q * VEC;  // row f * Kp of w, this thread's columns
  const float* __restrict__ c = coeff + (transpose ? j * Kp : j);
  const int cs = transpose ? 1 : Kp;
  float acc[VEC];
#pragma unroll
  for (int u = 0; u < VEC; ++u) acc[u] = 0.f;
  for (int i = 0; i < Kp; ++i) {
    const float ci = c[i * cs];
    float wi[VEC];
    ldv(wf + (int64_t)i * Fout, wi);
#pragma unroll
    for (int u = 0; u < VEC; ++u) acc[u] = fmaf(ci, wi[u], acc[u]);
  }
  stv(w_out + r * Fout + q * VEC, acc);
}

}  // namespace

}  // namespace dsph

extern "C" {

// every argument is checked here, before the launch
int dsph_basis_change(const float* w, const float* coeff, float* w_out, int32_t Fin, int32_t Fout, int32_t Kp, int32_t transpose,
                      int device, void* hip_stream) {
  using namespace dsph;
  if (!w || !coeff || !w_out) { set_error("basis_change: NULL pointer (w, coeff and w_out are required)"); return DSPH_E_BADARG; }
  if (Kp < 1 || Kp > 64) { set_error("basis_change: Kp = %d terms, must lie in [1, 64]", (int)Kp); return DSPH_E_BADARG; }
  if (Fin < 1 || Fout < 1) { set_error("basis_change: Fin = %d, Fout = %d, both must be at least 1", (int)Fin, (int)Fout); return DSPH_E_BADARG; }
  if (transpose != 0 && transpose != 1) { set_error("basis_change: transpose = %d, must be 0 or 1", (int)transpose); return DSPH_E_BADARG; }
  const int64_t elems = (int64_t)Fin * Kp * Fout;  // < 2^31 * 64 * 2^31: fits
  if (elems > ((int64_t)1 << 40)) { set_error("basis_change: Fin * Kp * Fout = %lld elements", (long long)elems); return DSPH_E_UNSUPPORTED; }
  const size_t bytes = (size_t)elems * sizeof(float);
  if (ranges_overlap(w, bytes, w_out, bytes)) {
    set_error("basis_change: w and w_out overlap; every output row reads Kp input rows and the map cannot run in place");
    return DSPH_E_BADARG;
  }
  if (ranges_overlap(coeff, (size_t)Kp * Kp * sizeof(float), w_out, bytes)) { set_error("basis_change: coeff and w_out overlap"); return DSPH_E_BADARG; }
  const int VEC = vec_width(Fout, ptr_bits({w, w_out}), true);
  const int64_t total = elems / VEC;
  const int64_t nblk = (total + 255) / 256;
  if (nblk > 0x7fffffffLL) { set_error("basis_change: grid too large (%lld workgroups)", (long long)nblk); return DSPH_E_UNSUPPORTED; }
  DeviceGuard guard(device);
  if (!select_device("basis_change", device, guard)) return DSPH_E_BADARG;
  DSPH_LAUNCH_BY_VEC(VEC, basis_change_kernel, dim3((unsigned)nblk), dim3(256), (hipStream_t)hip_stream, w, coeff, w_out, (int)Fout, (int)Kp,
                     (int)transpose, total);
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

}  // extern "C"
