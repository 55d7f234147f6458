// Host side of the strip kernel (cheb_strip_kernel.h): weight images, the cut of rectangles of class-R tiles
// into strip pairs, and the launch.
#include <algorithm>

#include "cheb_strip_kernel.h"

namespace dsph {

// Weight image of the strip kernel: one 1 KiB MFMA A-operand fragment per (role, ob, level of the role, ib, hi | lo);
// lane l, element e <- s_j * w[(16 ib + 8 (l >> 5) + e) * K + j][32 ob + (l & 31)], j the level (H: K-1-lev, L: S-1-lev),
// s_j the sign of the kept plane (sp_wsign).  Levels a role does not have are zero blocks.
__global__ __launch_bounds__(256) void strip_wprep_kernel(const float* __restrict__ w, unsigned char* __restrict__ out, int Fin,
                                                          int Fout, int K, int NIB, int NLEV, int cheb, int ld) {
  const int blk = blockIdx.x;  // ((role * 2 + ob) * NLEV + lev) * NIB + ib
  const int ib = blk % NIB, lev = (blk / NIB) % NLEV, ob = (blk / (NIB * NLEV)) & 1, role = blk / (NIB * NLEV * 2);
  const int S = K / 2;
  const int j = role == 0 ? K - 1 - lev : S - 1 - lev;
  const bool have = role == 0 ? lev < K - S : lev < S;
  const float sgn = sp_wsign(cheb != 0, j);
  unsigned char* base = out + (size_t)blk * 2 * SP_FRAG;
  for (int e = threadIdx.x; e < WF_ELEMS; e += 256) {
    const WfElem p = wf_elem32(e);
    wf_put(base, WF_BF16X3, p.l, p.j, have ? wf_gather(w, 16 * ib + p.inner, 32 * ob + p.col, Fin, Fout, K, j, ld, sgn) : 0.f);
  }
}

bool strip_shape_ok(int32_t Fin, int32_t Fout, int32_t K) {
  return K == 5 && Fin == 64 && Fout == 64;  // (cheb_strip5_kernel's shape)
}

size_t strip_wimg_bytes(int32_t Fin, int32_t Fout, int32_t K) {
  (void)Fout;
  const int NIB = (Fin + 15) / 16, S = K / 2, NLEV = std::max(K - S, S);
  return (size_t)2 * 2 * NLEV * NIB * 2 * SP_FRAG;
}

int launch_cheb_strip(const StripLaunch& s, hipStream_t stream) {
  if (s.K != 5) {  // (strip_shape_ok() admits nothing else; the weight image below is laid out for any K)
    set_error("cheb_strip: K = %d", s.K);
    return DSPH_E_UNSUPPORTED;
  }
  const int NIB = (s.Fin + 15) / 16, S = s.K / 2, NLEV = std::max(s.K - S, S);
  if (s.prep_weights) {
    hipLaunchKernelGGL(strip_wprep_kernel, dim3(2 * 2 * NLEV * NIB), dim3(256), 0, stream, s.w, s.wimg, (int)s.Fin, (int)s.Fout,
                       (int)s.K, NIB, NLEV, s.cheb ? 1 : 0, (int)s.ld);
    DSPH_HIP(hipGetLastError());
  }
  StripArgs a;
  a.x = s.x;
  a.bias = s.bias;
  a.y = s.y;
  a.wimg = s.wimg;
  a.gvals8 = s.gvals8;
  a.gdiag = s.gdiag;
  a.pairs = s.pairs;
  a.x_rows = s.x_rows;
  a.y_rows = s.y_rows;
  a.npairs = s.npairs;
  a.N = (int)s.N;
  a.Fin = s.Fin;
  a.Fout = s.Fout;
  a.ld = s.ld;
  a.act = s.act;
  // (one workgroup per CU, fewer when there are fewer (pair, map) items; cheb_tiles.hip's strip_makespan mirrors this)
  const int grid = (int)std::max<int64_t>(8, std::min<int64_t>(s.num_cu, ((int64_t)s.npairs * s.N + 7) / 8 * 8));
  hipLaunchKernelGGL(s.cheb ? cheb_strip5_kernel<true> : cheb_strip5_kernel<false>, dim3(grid), dim3(SP_THREADS), 0, stream, a);
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

}  // namespace dsph
