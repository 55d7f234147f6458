// What the quad-strip kernels share (cheb_qstrip_kernel.h: K = 5 forward, cheb_qstrip8_kernel.h: K = 8 forward,
// cheb_qwgrad_kernel.h: K = 5 weight gradient): the strip record and the lane's row types, the walk along the tape of strip
// rows, the rows through the rectangles' tables of tile bases, the step barrier and the LDS counters, the fp32 -> hi | lo split
// of an operand pair, the ring row of L~, the weight images' scale and fragment write, and the host's copy of a launch record
// into a kernel's arguments.  Each kernel keeps what is its own: roles, LDS layout, MFMA chains and step schedule.
//
// Everything here is __forceinline__ and takes what it needs as arguments: a kernel that calls it compiles to the instructions it
// had with the code written out in place.
#pragma once

#include <algorithm>

#include "cheb_struct_kernel.h"
#include "dsphere_common.h"

namespace dsph {

constexpr int QS_FRAG = 1024;                   // bytes of one MFMA operand fragment (64 lanes x 16 B)
constexpr int QS_CROWB = 2304;                  // one ring row of L~: [9: the diagonal, directions 0..7][p][tile] floats

typedef float qs_f4 __attribute__((ext_vector_type(4)));
typedef int qs_i4 __attribute__((ext_vector_type(4)));
typedef __bf16 qs_bf8 __attribute__((ext_vector_type(8)));
typedef unsigned qs_u2 __attribute__((ext_vector_type(2)));

// one row of a plane as a wave holds it: tile t = pixel 4 p + t, element e = output channel 16 oq + 4 (lane >> 4) + e
struct QRow {
  qs_f4 t[4];
};

// One work item (with a map of the batch): a strip of up to 56 output columns over rows [y0, y1).
struct QStrip {
  int32_t x0, w;      // virtual x of the first output column, output columns (<= QS_USE)
  int32_t xs;         // virtual x of column 0 (x0 - D; columns are clamped to [xlo, xhi] when loaded)
  int32_t y0, y1;     // output rows [y0, y1)
  int32_t xlo, xhi;   // the rectangle and its halo
  int32_t ylo, yhi;
  int32_t tab, tws;   // the rectangle's table of tile bases (offset into the kernel's `tab`) and its row stride: pixel (x, y) of the
                      // strip's plane is row tab[(y >> 4) * tws + (x >> 4)] + morton(x & 15, y & 15)
  int32_t img;        // the strip's first row of the packed image of L~ (qstrip_cimage_kernel): the row of y is img + y - (ylo - 1)
};

// ---- the tape ---------------------------------------------------------------------------------------------------------------
// The rows of all strips laid end to end form one tape per map (prefix[s] = rows of the strips before strip s, prefix[nstrips]
// = all rows); the host cuts it into `pieces` equal pieces and lets `wg_per_piece` workgroups share a piece, workgroup j of
// them taking the maps j, j + wg_per_piece, ... (qtape_split).
struct QTapePiece {
  int ord, piece, map0;  // the workgroup's place in the XCD-wise order, its piece of the tape and its first map
};
// (the workgroups of one XCD -- blockIdx & 7 -- are neighbours in `ord`; the host launches a multiple of 8)
__device__ __forceinline__ QTapePiece qt_piece(int wg_per_piece) {
  QTapePiece c;
  const int G = gridDim.x;
  c.ord = (blockIdx.x & 7) * (G >> 3) + (blockIdx.x >> 3);
  c.piece = c.ord / wg_per_piece;
  c.map0 = c.ord - c.piece * wg_per_piece;
  return c;
}
struct QTapeRange {
  int64_t begin, end;
};
// tape rows [begin, end) of a piece; a workgroup beyond the last piece gets an empty range (the forwards leave before they ask)
__device__ __forceinline__ QTapeRange qt_tape_range(const int32_t* prefix, int nstrips, int piece, int pieces) {
  const int64_t tape = (int64_t)prefix[nstrips];
  QTapeRange r;
  r.begin = piece < pieces ? tape * piece / pieces : 0;
  r.end = piece < pieces ? tape * (piece + 1) / pieces : 0;
  return r;
}
// the run of rows that starts at tape row r: its strip, cut to [r, r_end) (wave-uniform arithmetic); returns its length
__device__ __forceinline__ int qt_locate(const int32_t* prefix, const QStrip* strips, int nstrips, int64_t r, int64_t r_end, QStrip& st) {
  int lo = 0, hi = nstrips;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)prefix[mid] <= r) lo = mid; else hi = mid;
  }
  {  // (the record through scalar registers: every field is wave-uniform, and the compiler should know -- rows, clamps and the
     // table look-ups' branches then run on the scalar unit)
    const QStrip g = strips[lo];
#define QS_U(f) st.f = __builtin_amdgcn_readfirstlane(g.f)
    QS_U(x0); QS_U(w); QS_U(xs); QS_U(y0); QS_U(y1); QS_U(xlo); QS_U(xhi); QS_U(ylo); QS_U(yhi); QS_U(tab); QS_U(tws); QS_U(img);
#undef QS_U
  }
  const int h = st.y1 - st.y0;
  const int off = (int)(r - (int64_t)prefix[lo]);
  const int len = (int)(((int64_t)(h - off) < r_end - r) ? (int64_t)(h - off) : r_end - r);
  st.y0 += off;
  st.y1 = st.y0 + len;
  return len;
}

// ---- rows through the table of tile bases -------------------------------------------------------------------------------------
// Where a pixel of the strip's plane lives: row = tab[(y >> 4) tws + (x >> 4)] + morton(x & 15, y & 15) -- the rectangle's table
// of tile bases (cheb_tiles.hip, build_qtstrips: a rectangle may cross base-pixel borders that continue the pixel grid by a
// translation; inside a base pixel the table is the Morton plane itself).  A strip's 64 columns lie in at most five tile
// columns, the row y is wave-uniform: the five bases of a tile row come by SCALAR loads (they share no counter with the
// vector memory: a vector load here would wait for the previous step's y stores to drain -- measured, 12 % of the forward),
// a lane keeps the one of its column (ci = its tile column - the strip's first) -- looked up when a row enters a new tile
// row, every sixteenth step.  yc: the row, clamped by the caller to the rows its operand has.
__device__ __forceinline__ unsigned qt_tab_lane(const int32_t* tab, const QStrip& st, unsigned ci, int yc) {
  const int32_t* trow = tab + __builtin_amdgcn_readfirstlane(st.tab + (yc >> 4) * st.tws + (max(st.xs, st.xlo) >> 4));
  qs_i4 b;
  int b4;
  asm volatile("s_load_dwordx4 %0, %2, 0x0\n\ts_load_dword %1, %2, 0x10\n\ts_waitcnt lgkmcnt(0)" : "=&s"(b), "=&s"(b4) : "s"(trow) : "memory");
  return (unsigned)(ci == 0 ? b[0] : ci == 1 ? b[1] : ci == 2 ? b[2] : ci == 3 ? b[3] : b4);
}
// the row of pixel (column with Morton bits mX, row yrow clamped to the rectangle and its halo) in the tile at `base`
__device__ __forceinline__ unsigned qt_row_in(const QStrip& st, unsigned base, unsigned mX, int yrow) {
  const int yc = min(max(yrow, st.ylo), st.yhi);
  return base + (mX | (st_spread((unsigned)yc & 15u) << 1));
}

// ---- the step's barrier and the hand-over counters in LDS -------------------------------------------------------------------
__device__ __forceinline__ void qt_step_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
__device__ __forceinline__ void qt_flag_set(unsigned addr, int v) { asm volatile("ds_write_b32 %0, %1" : : "v"(addr), "v"(v) : "memory"); }
__device__ __forceinline__ int qt_flag_get(unsigned addr) {
  int v;
  asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(addr) : "memory");
  return v;
}

// ---- fp32 pair -> hi | lo -------------------------------------------------------------------------------------------------------
// Two neighbouring values as an MFMA operand holds them: [0] = the pair's high parts, [1] = what they leave, each two bf16 (8 + 8
// mantissa bits) or two f16 (11 + 11: DSPH_PREC_F16X3).
template <bool F16> __device__ __forceinline__ qs_u2 qt_split(float a0, float a1) {
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  qs_u2 r;
  if (F16) {  // (a value beyond the f16 range becomes an infinity here and a NaN row in y: loud, not wrong)
    const f16x2 h = __builtin_convertvector(f32x2{a0, a1}, f16x2);
    const f32x2 hf = __builtin_convertvector(h, f32x2);
    const f16x2 l = __builtin_convertvector(f32x2{a0 - hf[0], a1 - hf[1]}, f16x2);
    r[0] = __builtin_bit_cast(unsigned, h);
    r[1] = __builtin_bit_cast(unsigned, l);
  } else {
    const bf16x2 h = __builtin_convertvector(f32x2{a0, a1}, bf16x2);
    const unsigned hu = __builtin_bit_cast(unsigned, h);
    const float h0 = __builtin_bit_cast(float, hu << 16), h1 = __builtin_bit_cast(float, hu & 0xffff0000u);
    const bf16x2 l = __builtin_convertvector(f32x2{a0 - h0, a1 - h1}, bf16x2);
    r[0] = hu;
    r[1] = __builtin_bit_cast(unsigned, l);
  }
  return r;
}

// ---- the ring row of L~ -------------------------------------------------------------------------------------------------------
// The values of L~ of the lane's four pixels in one row, as the ring holds them: vector v = 0 the diagonal, v = 1 + d direction d
// (W NW N NE E SE S SW: kDirX / kDirY order), each a [p][tile] vector of 256 bytes -- what a lane reads is the 16 bytes of its
// four pixels of one direction.  A source row takes three of them (west, centre, east by tile):
//   y-1: SW S SE;  y: W diag E;  y+1: NW N NE.
struct QCoef3 {
  qs_f4 w, c, e;
};
struct QCoefLo {  // what the rows y-1 and y of a level need: six directions, each a vector by tile
  qs_f4 sw, s, se, w, dg, e;
};
struct QCoefHi {  // what the row y+1 needs
  qs_f4 nw, n, ne;
};
// coefficient vectors of the three source rows
#define QS_LO0(c) (c).sw, (c).s, (c).se
#define QS_LO1(c) (c).w, (c).dg, (c).e
#define QS_HI(c) (c).nw, (c).n, (c).ne

// row `rid` of L~ from global memory: lanes q4 = 0 (and 2) take the directions 0..3, q4 = 1 (and 3) 4..7, every lane the diagonal
__device__ __forceinline__ void qt_cfetch(const float* gvals8, const float* gdiag, size_t rid, int q4, qs_f4& cv, float& cd) {
  const char* pv = reinterpret_cast<const char*>(gvals8) + rid * 32u + (unsigned)(q4 & 1) * 16u;
  const char* pd = reinterpret_cast<const char*>(gdiag) + rid * 4u;
  cv = *reinterpret_cast<const qs_f4*>(pv);
  cd = *reinterpret_cast<const float*>(pd);
}
// ... filed in slot `slot` of the ring at `ring` as the values of the pixels 4 p + res; DOUBLE: as 2 L~ (Chebyshev recurrence)
template <bool DOUBLE>
__device__ __forceinline__ void qt_cstore(unsigned char* ring, int slot, int p, int q4, int res, qs_f4 cv, float cd) {
  if (DOUBLE) { cv = cv + cv; cd = cd + cd; }
  unsigned char* q = ring + (unsigned)slot * QS_CROWB + (unsigned)p * 16u + (unsigned)res * 4u;
  if (q4 < 2) {
#pragma unroll
    for (int d = 0; d < 4; ++d) *reinterpret_cast<float*>(q + (unsigned)(1 + 4 * q4 + d) * 256u) = cv[d];
  }
  if (q4 == 2) *reinterpret_cast<float*>(q) = cd;
}
// ... or a quarter of it straight from the packed image (cheb_qstrip.hip, qstrip_cimage_kernel) by LDS-DMA: `row` is the image
// row (wave-uniform), voff the lane's byte in it, lds_dst the quarter's place in the ring slot (wave-uniform); 36 lanes x 16 bytes.
// The issuing wave calls qt_wait_vm() in front of the barrier that publishes the row.
__device__ __forceinline__ void qt_cdma(const unsigned char* row, unsigned voff, unsigned lds_dst, int lane) {
  if (lane < QS_CROWB / 4 / 16) st_glds16_off(row, voff, lds_dst);
}
__device__ __forceinline__ void qt_wait_vm() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// the lane's part of a ring row, and vector v of it (NOREAD: a tuning build's cut -- a constant instead of the LDS read)
__device__ __forceinline__ const unsigned char* qt_crow(const unsigned char* ring, int slot, int p) {
  return ring + (unsigned)slot * QS_CROWB + (unsigned)p * 16u;
}
template <bool NOREAD = false> __device__ __forceinline__ qs_f4 qt_cvec(const unsigned char* q, int v) {
  if (NOREAD) { qs_f4 c = qs_f4{0.1f, 0.1f, 0.1f, 0.1f}; asm volatile("" : "+v"(c)); return c; }
  return *reinterpret_cast<const qs_f4*>(q + (unsigned)v * 256u);
}
// the three vectors of the source row y-1 (which = 0), y (1), y+1 (2)
template <bool NOREAD = false> __device__ __forceinline__ QCoef3 qt_cvec3(const unsigned char* q, int which) {
  QCoef3 r;
  if (which == 0) { r.w = qt_cvec<NOREAD>(q, 8); r.c = qt_cvec<NOREAD>(q, 7); r.e = qt_cvec<NOREAD>(q, 6); }
  else if (which == 1) { r.w = qt_cvec<NOREAD>(q, 1); r.c = qt_cvec<NOREAD>(q, 0); r.e = qt_cvec<NOREAD>(q, 5); }
  else { r.w = qt_cvec<NOREAD>(q, 2); r.c = qt_cvec<NOREAD>(q, 3); r.e = qt_cvec<NOREAD>(q, 4); }
  return r;
}
template <bool NOREAD = false> __device__ __forceinline__ QCoefLo qt_clo_read(const unsigned char* ring, int slot, int p) {
  const unsigned char* q = qt_crow(ring, slot, p);
  QCoefLo c;
  c.sw = qt_cvec<NOREAD>(q, 8); c.s = qt_cvec<NOREAD>(q, 7); c.se = qt_cvec<NOREAD>(q, 6);
  c.w = qt_cvec<NOREAD>(q, 1); c.dg = qt_cvec<NOREAD>(q, 0); c.e = qt_cvec<NOREAD>(q, 5);
  return c;
}
template <bool NOREAD = false> __device__ __forceinline__ QCoefHi qt_chi_read(const unsigned char* ring, int slot, int p) {
  const unsigned char* q = qt_crow(ring, slot, p);
  QCoefHi c;
  c.nw = qt_cvec<NOREAD>(q, 2); c.n = qt_cvec<NOREAD>(q, 3); c.ne = qt_cvec<NOREAD>(q, 4);
  return c;
}

// ---- the forwards' weight images (one block of 256 threads per pair of hi | lo A fragments) ------------------------------------
// f16 images carry the weights times the power of two that puts the largest of the nrows x ncols in [2048, 4096) -- lo parts
// stay normal numbers --; every block finds the same maximum.  Returns that power (1 for all-zero or non-finite weights).
__device__ __forceinline__ float qt_wimg_pow2(const float* __restrict__ w, int nrows, int ncols, int ld) {
  __shared__ float smax[256];
  float m = 0.f;
  for (int e = threadIdx.x; e < nrows * ncols; e += 256) m = fmaxf(m, fabsf(w[(int64_t)(e / ncols) * ld + e % ncols]));
  smax[threadIdx.x] = m;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) smax[threadIdx.x] = fmaxf(smax[threadIdx.x], smax[threadIdx.x + st]);
    __syncthreads();
  }
  int ex = 0;
  const float mx = smax[0];
  float pw = 1.f;
  if (mx > 0.f && mx < 3.0e38f) { (void)frexpf(mx, &ex); pw = ldexpf(1.f, 12 - ex); }  // mx = f 2^ex, f in [0.5, 1): mx pw in [2048, 4096)
  return pw;
}
// (the elements go in through wf_put of dsphere_wfrag.h: WF_BF16X3 or WF_F16X3)

// ---- host: a launch record into a kernel's arguments ------------------------------------------------------------------------
// What QStripArgs, Q8Args and QWgradArgs have in common, and the cut of the tape with the kernel's run-in; returns the grid.
template <class Args, class Launch> int qtape_args(Args& a, const Launch& s, int run_in) {
  a.x = s.x;
  a.gvals8 = s.gvals8;
  a.gdiag = s.gdiag;
  a.strips = s.strips;
  a.tab = s.tab;
  a.prefix = s.prefix;
  a.x_rows = s.x_rows;
  a.nstrips = s.nstrips;
  a.N = (int)s.N;
  int grid;
  (void)qtape_split(s.num_cu, s.tape_rows, s.N, s.tape_rows / std::max(1, s.nstrips), run_in, &grid, &a.pieces, &a.wg_per_piece);
  return grid;
}
// ... and what the two forwards' have on top
template <class Args> int qtape_forward_args(Args& a, const QTapeLaunch& s, int run_in) {
  a.bias = s.bias;
  a.y = s.y;
  a.wimg = s.wimg;
  a.y_rows = s.y_rows;
  a.ld = s.ld;
  a.act = s.act;
  a.xsc = s.f16 ? ldexpf(1.f, s.f16_xexp) : 1.f;
  a.xsc_inv = s.f16 ? ldexpf(1.f, -s.f16_xexp) : 1.f;
  return qtape_args(a, s, run_in);
}

}  // namespace dsph
