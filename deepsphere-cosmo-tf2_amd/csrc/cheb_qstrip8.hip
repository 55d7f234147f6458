// Host side of the K = 8 quad-strip kernel (cheb_qstrip8_kernel.h): weight image and launch.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "cheb_qstrip8_kernel.h"
#include "dsphere_wfrag.h"

namespace dsph {

// Weight image: one 1 KiB A-operand fragment of v_mfma_f32_16x16x32_bf16 per (role, quarter oq, level of the role, hi | lo): lane
// l, element i <- s_j m_j w[(8 (l >> 4) + i) * K + j][16 oq + (l & 15)], j the level (top 7 - lev, middle 4 - lev, bottom 1 - lev),
// s_j the sign kept with the plane (qs_wsign), m_0 = 2 (level 0 runs doubled: the kernel halves y when it stores it).  The third
// level of `bottom` is a zero block.
__global__ __launch_bounds__(256) void qstrip8_wprep_kernel(const float* __restrict__ w, unsigned char* __restrict__ out, int ld, int f16) {
  constexpr int K = Q8_K;
  const int blk = blockIdx.x;  // (role * 2 + oq) * 3 + lev
  const int lev = blk % 3, oq = (blk / 3) & 1, role = blk / 6;
  const int j = (role == 0 ? 7 : role == 1 ? 4 : 1) - lev;
  const bool have = j >= 0;
  float sc = have ? qs_wsign(true, j) * (j == 0 ? 2.f : 1.f) : 0.f;
  if (f16) {
    const float pw = qt_wimg_pow2(w, 32 * K, 32, ld);
    sc *= pw;
    if (blk == 0 && threadIdx.x == 0) *reinterpret_cast<float*>(out + (size_t)Q8_WIMG) = 1.f / pw;
  }
  unsigned char* base = out + (size_t)blk * 2 * QS_FRAG;
  for (int e = threadIdx.x; e < WF_ELEMS; e += 256) {
    const WfElem p = wf_elem16(e);
    wf_put(base, f16 ? WF_F16X3 : WF_BF16X3, p.l, p.j, have ? wf_gather(w, p.inner, 16 * oq + p.col, 32, 32, K, j, ld, sc) : 0.f);
  }
}

bool qstrip8_shape_ok(int32_t Fin, int32_t Fout, int32_t K) { return K == Q8_K && Fin == 32 && Fout == 32; }
size_t qstrip8_wimg_bytes() { return (size_t)Q8_WIMG + 256; }  // (+ the f16 image's factor)

// The tape of rows is cut as for the K = 5 kernel (qtape_split) with this kernel's run-in; a single map (configs[3]) is one
// workgroup per piece.
int64_t qstrip8_split(int num_cu, int64_t tape_rows, int64_t N, int64_t mean_height, int* grid, int* pieces, int* wg_per_piece) {
  return qtape_split(num_cu, tape_rows, N, mean_height, Q8_RUNIN, grid, pieces, wg_per_piece);
}

int launch_cheb_qstrip8(const QStrip8Launch& s, hipStream_t stream) {
  if (s.prep_weights) {
    hipLaunchKernelGGL(qstrip8_wprep_kernel, dim3(3 * 2 * 3), dim3(256), 0, stream, s.w, s.wimg, (int)s.ld_w, s.f16 ? 1 : 0);
    DSPH_HIP(hipGetLastError());
  }
  Q8Args a;
  const int grid = qtape_forward_args(a, s, Q8_RUNIN);
#ifdef DSPH_Q8_SIX_WAVES  // (tuning: the six-wave variant, `top` fetching)
  if (s.f16) hipLaunchKernelGGL((cheb_qstrip8_kernel<0, true>), dim3(grid), dim3(Q8_THREADS), 0, stream, a);
  else hipLaunchKernelGGL((cheb_qstrip8_kernel<0, false>), dim3(grid), dim3(Q8_THREADS), 0, stream, a);
#else
  if (s.f16) hipLaunchKernelGGL((cheb_qstrip8_kernel<1, true>), dim3(grid), dim3(512), 0, stream, a);
  else hipLaunchKernelGGL((cheb_qstrip8_kernel<1, false>), dim3(grid), dim3(512), 0, stream, a);
#endif
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

}  // namespace dsph
