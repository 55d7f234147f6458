// Host side of the quad-strip kernel (cheb_qstrip_kernel.h): weight image and launch.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "cheb_qstrip_kernel.h"
#include "dsphere_wfrag.h"

namespace dsph {

// Weight image: one 1 KiB A-operand fragment of v_mfma_f32_16x16x32_{bf16,f16} per (role, quarter oq, level of the role,
// 32-channel block kb, hi | lo): lane l, element i <- s_j m_j w[(32 kb + 8 (l >> 4) + i) * K + j][16 oq + (l & 15)], j the level
// (H: 4 - lev, L: 1 - lev), s_j the sign kept with the plane (qs_wsign), m_0 = 2 in the Chebyshev basis (level 0 runs doubled:
// the kernel halves y when it stores it).  The third level of role L is a zero block.
// f16 (DSPH_PREC_F16X3): hi | lo are f16 (11 + 11 mantissa bits), the weights times the power of two that puts the largest
// one in [2048, 4096) -- lo parts stay normal numbers --; the inverse factor sits behind the fragments for the kernel's store.
__global__ __launch_bounds__(256) void qstrip_wprep_kernel(const float* __restrict__ w, unsigned char* __restrict__ out, int Fin,
                                                           int Fout, int cheb, int ld, int f16) {
  constexpr int K = 5;
  const int blk = blockIdx.x;  // ((role * 4 + oq) * 3 + lev) * 2 + kb
  const int kb = blk & 1, lev = (blk >> 1) % 3, oq = ((blk >> 1) / 3) & 3, role = (blk >> 1) / 12;
  const int j = role == 0 ? K - 1 - lev : 1 - lev;
  const bool have = role == 0 || lev < 2;
  float sc = qs_wsign(cheb != 0, j) * ((cheb != 0 && j == 0) ? 2.f : 1.f);
  if (f16) {
    const float pw = qt_wimg_pow2(w, Fin * K, Fout, ld);
    sc *= pw;
    if (blk == 0 && threadIdx.x == 0) *reinterpret_cast<float*>(out + (size_t)2 * 4 * 3 * 2 * 2 * QS_FRAG) = 1.f / pw;
  }
  unsigned char* base = out + (size_t)blk * 2 * QS_FRAG;
  for (int e = threadIdx.x; e < WF_ELEMS; e += 256) {
    const WfElem p = wf_elem16(e);
    wf_put(base, f16 ? WF_F16X3 : WF_BF16X3, p.l, p.j, have ? wf_gather(w, 32 * kb + p.inner, 16 * oq + p.col, Fin, Fout, K, j, ld, sc) : 0.f);
  }
}

// The packed image of L~ (QStripArgs::cimg): for every strip the ring rows of the steps y = ylo - 1 .. yhi + 6 -- every row a run
// of steps can ask for, the rows dsph_plan_strip_rows answers for --, each as the H waves filed it from gvals8 / gdiag: QS_CROWB
// bytes, [diagonal, directions 0..7][p][tile] floats, the values of the pixel in column clamp(xs + 4 p + tile, xlo, xhi) found
// through the strip's table of tile bases; doubled for the Chebyshev recurrence (dbl).  A constant of the plan: built once (after
// struct_patch_rows: it holds the patched class-T values), read by every step of every forward.  One block per image row.
__global__ __launch_bounds__(256) void qstrip_cimage_kernel(const QStrip* __restrict__ strips, int nstrips, const int32_t* __restrict__ tab,
                                                            const float* __restrict__ gvals8, const float* __restrict__ gdiag,
                                                            int64_t rows, int dbl, float* __restrict__ out) {
  for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
    int lo = 0, hi = nstrips;  // the strip of image row r: the last one that starts at or before it
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if ((int64_t)strips[mid].img <= r) lo = mid; else hi = mid;
    }
    const QStrip st = strips[lo];
    const int y = st.ylo - 1 + (int)(r - st.img);
    for (int e = threadIdx.x; e < QS_CROWB / 4; e += 256) {
      const int v = e >> 6, p = (e >> 2) & 15, t = e & 3;
      const int x = min(max(st.xs + 4 * p + t, st.xlo), st.xhi);
      const size_t rid = (size_t)tab[st.tab + (y >> 4) * st.tws + (x >> 4)] + st_morton((unsigned)x & 15u, (unsigned)y & 15u);
      const float c = v == 0 ? gdiag[rid] : gvals8[rid * 8 + (size_t)(v - 1)];
      out[r * (QS_CROWB / 4) + e] = dbl ? c + c : c;
    }
  }
}
int64_t qstrip_cimage_rows(const QStrip& q) { return (int64_t)q.yhi - q.ylo + 8; }
int launch_qstrip_cimage(const QStrip* d_strips, int nstrips, const int32_t* d_tab, const float* gvals8, const float* gdiag, int64_t rows,
                         bool doubled, float* d_out, hipStream_t stream) {
  if (rows <= 0) return DSPH_OK;
  hipLaunchKernelGGL(qstrip_cimage_kernel, dim3((unsigned)std::min<int64_t>(rows, 1 << 16)), dim3(256), 0, stream, d_strips, nstrips, d_tab,
                     gvals8, gdiag, rows, doubled ? 1 : 0, d_out);
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

bool qstrip_shape_ok(int32_t Fin, int32_t Fout, int32_t K) { return K == 5 && Fin == 64 && Fout == 64; }

// The split rule of the quad-strip kernels (dsphere_common.h)
int64_t qtape_split(int num_cu, int64_t tape_rows, int64_t N, int64_t mean_height, int run_in, int* grid, int* pieces, int* wg_per_piece) {
  const int g = (int)std::max<int64_t>(8, std::min<int64_t>(num_cu / 8 * 8, tape_rows * N / 64 / 8 * 8));
  auto span_of = [&](int64_t w) {
    const int64_t P = std::max<int64_t>(1, g / w), share = (tape_rows + P - 1) / P, maps = (N + w - 1) / w;
    const int64_t runs = share / std::max<int64_t>(1, mean_height) + 2;
    return (share + runs * (run_in + 1)) * maps;
  };
  int64_t best_w = 1, best = -1;
  if (N <= g) { best_w = N; best = span_of(N); }
  else
    for (int64_t w = 1; w <= g; w *= 2) {
      const int64_t sp = span_of(w);
      if (best < 0 || sp < best) { best = sp; best_w = w; }
    }
  if (grid) *grid = g;
  if (pieces) *pieces = (int)std::max<int64_t>(1, g / best_w);
  if (wg_per_piece) *wg_per_piece = (int)best_w;
  return best;
}
int64_t qstrip_split(int num_cu, int64_t tape_rows, int64_t N, int64_t mean_height, int* grid, int* pieces, int* wg_per_piece) {
  return qtape_split(num_cu, tape_rows, N, mean_height, QS_RUNIN, grid, pieces, wg_per_piece);
}

size_t qstrip_wimg_bytes() { return (size_t)2 * 4 * 3 * 2 * 2 * QS_FRAG + 256; }  // 96 KiB + the f16 image's factor

int launch_cheb_qstrip(const QStripLaunch& s, hipStream_t stream) {
  if (s.prep_weights) {
    hipLaunchKernelGGL(qstrip_wprep_kernel, dim3(2 * 4 * 3 * 2), dim3(256), 0, stream, s.w, s.wimg, (int)s.Fin, (int)s.Fout, s.cheb ? 1 : 0,
                       (int)s.ld, s.f16 ? 1 : 0);
    DSPH_HIP(hipGetLastError());
  }
  QStripArgs a;
  a.Fin = s.Fin;
  a.Fout = s.Fout;
  a.cimg = s.cimg;
  const int grid = qtape_forward_args(a, s, QS_RUNIN);
  void (*kern)(QStripArgs);
  if (s.cimg) kern = s.f16 ? (s.cheb ? cheb_qstrip5_kernel<true, true, true> : cheb_qstrip5_kernel<false, true, true>)
                           : (s.cheb ? cheb_qstrip5_kernel<true, false, true> : cheb_qstrip5_kernel<false, false, true>);
  else kern = s.f16 ? (s.cheb ? cheb_qstrip5_kernel<true, true, false> : cheb_qstrip5_kernel<false, true, false>)
                    : (s.cheb ? cheb_qstrip5_kernel<true, false, false> : cheb_qstrip5_kernel<false, false, false>);
#ifdef DSPH_QS_STAMPS
  static unsigned* d_stamps = nullptr;
  constexpr size_t NST = 8 * 4 * 10;
  if (!d_stamps) DSPH_HIP(hipMalloc(&d_stamps, NST * 4));
  DSPH_HIP(hipMemsetAsync(d_stamps, 0, NST * 4, stream));
  a.stamps = d_stamps;
#endif
  hipLaunchKernelGGL(kern, dim3(grid), dim3(QS_THREADS), 0, stream, a);
  DSPH_HIP(hipGetLastError());
#ifdef DSPH_QS_STAMPS
  if (getenv("DSPH_STAMPS_DUMP")) {
    std::vector<unsigned> h(NST);
    if (hipStreamSynchronize(stream) == hipSuccess && hipMemcpy(h.data(), d_stamps, NST * 4, hipMemcpyDeviceToHost) == hipSuccess)
      for (int w = 0; w < 8; ++w)
        for (int it = 0; it < 4; ++it) {
          const unsigned* r = &h[((size_t)w * 4 + it) * 10];
          fprintf(stderr, "QSSTAMP wave %d step %2d:", w, it);
          unsigned prev = r[0];
          for (int i = 1; i <= 8; ++i) {
            if (r[i] == 0) { fprintf(stderr, "      -"); continue; }
            fprintf(stderr, " %6u", r[i] - prev);
            prev = r[i];
          }
          fprintf(stderr, " | step %u | t0 %u\n", r[8] - r[0], r[0]);
        }
  }
#endif
  return DSPH_OK;
}

}  // namespace dsph
