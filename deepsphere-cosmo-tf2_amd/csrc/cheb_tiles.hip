// Host side of the fused path: the tile tables of a plan (cheb_tiles.h) and the queries of the C ABI that read them.  No kernel.
// get_tiles builds the tables of one depth in stages (build_tiles): classify, sort_tiles (class T by embed_tile, breadth-first
// tables of class G), merge_small_map, pair_strips, quad_strips5, quad_strips8, complements, upload_tables.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>

#include "cheb_tiles.h"

namespace dsph {

// the eight neighbouring cells / tiles, in the order of kDirX / kDirY (W NW N NE E SE S SW)
static const int ddx[8] = {-1, -1, 0, 1, 1, 1, 0, -1}, ddy[8] = {0, 1, 1, 1, 0, -1, -1, -1};

static int template_width(int w) {
  if (w <= 9) return 9;
  if (w <= 12) return 12;
  return 0;
}

static void cimage_free(const QStripSet& s) {
  for (float*& p : s.d_cimg) {
    if (p) (void)hipFree(p);
    p = nullptr;
  }
  s.cimg_failed = false;
}

void FusedTiles::release() {
  for (void* p : dev) (void)hipFree(p);
  cimage_free(q5);
  *this = FusedTiles();
}

FusedPlan* fused_plan_build(const dsph_plan* plan, const int32_t* h_cols, const float* h_vals) {
  if (template_width(plan->width) == 0 && tstep_width(plan->width) == 0) return nullptr;
  FusedPlan* fp = new FusedPlan();
  fp->wide = template_width(plan->width) == 0;
  const size_t nnz = (size_t)plan->n_rows * plan->width;
  fp->h_cols.assign(h_cols, h_cols + nnz);
  fp->h_vals.assign(h_vals, h_vals + nnz);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, plan->device) == hipSuccess && prop.multiProcessorCount > 0)
    fp->num_cu = prop.multiProcessorCount;
  return fp;
}

void fused_plan_destroy(FusedPlan* fp) {
  if (!fp) return;
  for (auto& kv : fp->by_depth) kv.second.release();
  if (fp->d_gvals8) (void)hipFree(fp->d_gvals8);
  if (fp->d_gdiag) (void)hipFree(fp->d_gdiag);
  if (fp->d_rowflag) (void)hipFree(fp->d_rowflag);
  if (fp->side) {
    (void)hipStreamSynchronize(fp->side);
    (void)hipEventDestroy(fp->ev_fork);
    (void)hipEventDestroy(fp->ev_join);
    (void)hipStreamDestroy(fp->side);
  }
  delete fp;
}

bool fused_host_released(FusedPlan* fp) {
  std::lock_guard<std::mutex> lock(fp->mu);
  return fp->host_released;
}

// The tile tables depend on which rows are outputs (dsph_plan_set_levels): drop the cached ones.
void fused_plan_invalidate(FusedPlan* fp) {
  if (!fp) return;
  std::lock_guard<std::mutex> lock(fp->mu);
  for (auto& kv : fp->by_depth) kv.second.release();
  fp->by_depth.clear();
}

// DSPH_OPT_QSTRIP_IMAGE changed: the images go (hipFree waits for the kernels that read them); the next forward decides anew
void fused_cimage_drop(FusedPlan* fp) {
  if (!fp) return;
  std::lock_guard<std::mutex> lock(fp->mu);
  for (auto& kv : fp->by_depth) cimage_free(kv.second.q5);
}

const float* qstrip_cimage(const dsph_plan* plan, const FusedTiles& ft, bool cheb, hipStream_t stream) {
  const QStripSet& s = ft.q5;
  if (plan->opt.qstrip_image == 2 || s.n == 0 || s.cimg_rows == 0) return nullptr;
  FusedPlan* fp = plan->fused;
  std::lock_guard<std::mutex> lock(fp->mu);
  float*& img = s.d_cimg[cheb ? 1 : 0];
  if (img || s.cimg_failed) return img;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (stream && (hipStreamIsCapturing(stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone)) return nullptr;
  void* p = nullptr;
  if (hipMalloc(&p, (size_t)s.cimg_rows * QS_CROWB) != hipSuccess) {
    (void)hipGetLastError();
    s.cimg_failed = true;
    return nullptr;
  }
  // (on the null stream and waited for: whichever stream the forwards run on finds the image complete)
  if (launch_qstrip_cimage(s.d_strips, s.n, s.d_tab, fp->d_gvals8, fp->d_gdiag, s.cimg_rows, cheb, static_cast<float*>(p), nullptr) != DSPH_OK ||
      hipStreamSynchronize(nullptr) != hipSuccess) {
    (void)hipFree(p);
    s.cimg_failed = true;
    return nullptr;
  }
  img = static_cast<float*>(p);
  return img;
}

// Class-T tiles: a tile whose own 256 rows are a 16x16 Morton square and whose D-ring region can be laid out as a
// (16+2D)^2 square of a 9-point stencil although the ROW NUMBERS of the halo are not a Morton continuation (the next base
// pixel of the sphere, possibly rotated; the halo rows of a sharded plan, numbered by hop distance).  The layout is
// found from the graph alone, ring by ring: a new cell is the one row that all of its already-placed neighbours have in
// common and that is not placed yet.  It is then VERIFIED, not trusted: every row that a step evaluates (rings 0..D-1)
// must have each non-zero of L~ on itself or on one of its eight neighbouring cells; only then do the tables exist.
// Anything else (the eight 7-neighbour corners of the sphere, mask edges, ragged tiles, k-NN graphs) stays class G.
// row: [ST_CELLS] row of every plane cell (plane-cell order, pads and cells outside the region: the tile's first row);
// val: [ST_CELLS][ST_TABV] diagonal, then the directions in the order of kDirX / kDirY.
static bool embed_tile(const dsph_plan* plan, const int32_t* cols, const float* vals, int W, int t, int D, int64_t out_rows,
                       int32_t* row, float* val, bool* interior, std::vector<int32_t>& key, std::vector<int32_t>& slot) {
  const int64_t r0 = (int64_t)t * FUSED_P;
  if (r0 + FUSED_P > out_rows) return false;  // ragged last tile
  constexpr int S = ST_S;
  int32_t A[S][S];
  for (int y = 0; y < S; ++y)
    for (int x = 0; x < S; ++x) A[x][y] = -1;
  // open-addressing map row -> cell (x + S * y); 2048 slots for at most 576 entries
  constexpr int HN = 2048;
  key.assign(HN, -1);
  slot.assign(HN, 0);
  auto hput = [&](int32_t r, int cell) {
    unsigned h = ((unsigned)r * 2654435761u) >> 21;
    while (key[h] != -1) h = (h + 1) & (HN - 1);
    key[h] = r;
    slot[h] = cell;
  };
  auto hget = [&](int32_t r) -> int {
    unsigned h = ((unsigned)r * 2654435761u) >> 21;
    while (key[h] != -1) {
      if (key[h] == r) return slot[h];
      h = (h + 1) & (HN - 1);
    }
    return -1;
  };
  for (unsigned y = 0; y < 16; ++y)
    for (unsigned x = 0; x < 16; ++x) {
      const int32_t r = (int32_t)(r0 + st_morton(x, y));
      A[ST_DMAX + x][ST_DMAX + y] = r;
      hput(r, (ST_DMAX + x) + S * (ST_DMAX + y));
    }
  // the one unplaced row adjacent to every placed neighbour of cell (x, y); -1 if there is none or more than one
  auto propose = [&](int x, int y) -> int32_t {
    int32_t cand[16];
    int nc = -1;  // -1: no anchor seen yet
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int ax = x + dx, ay = y + dy;
        if ((dx == 0 && dy == 0) || ax < 0 || ay < 0 || ax >= S || ay >= S || A[ax][ay] < 0) continue;
        const int32_t ar = A[ax][ay];
        if (ar >= plan->n_rows) continue;  // an input-only row has no list of neighbours: not an anchor
        const int32_t* c = cols + (size_t)ar * W;
        const float* v = vals + (size_t)ar * W;
        if (nc < 0) {
          nc = 0;
          for (int j = 0; j < W; ++j)
            if (v[j] != 0.f && c[j] != ar && hget(c[j]) < 0 && nc < 16) cand[nc++] = c[j];
        } else {
          int m = 0;
          for (int i = 0; i < nc; ++i) {
            bool in = false;
            for (int j = 0; j < W && !in; ++j) in = v[j] != 0.f && c[j] == cand[i];
            if (in) cand[m++] = cand[i];
          }
          nc = m;
        }
      }
    return nc == 1 ? cand[0] : (nc > 1 ? -1 : -2);  // -1: ambiguous; -2: no row belongs here
  };
  // A cell no row belongs to is a HOLE (round 6: the edge of a survey mask -- the pixel beyond it does not exist): it stays
  // negative in A (never an anchor), its table entry is the tile's first row with nine zeros -- what a step computes there is
  // finite and no row of the map has a non-zero towards it.  Nothing is taken on trust: the verification below still demands
  // that every non-zero of every evaluated row lands on a placed cell at one of the eight offsets, so a row left out by
  // mistake (or a vertex where three base pixels meet, whose far seam is not a 3 x 3 neighbourhood) fails the tile as before.
  auto place = [&](int x, int y) -> bool {
    const int32_t r = propose(x, y);
    if (r == -1) return false;
    if (r == -2) { A[x][y] = -2; return true; }
    A[x][y] = r;
    hput(r, x + S * y);
    return true;
  };
  for (int rho = 1; rho <= D; ++rho) {
    const int lo = ST_DMAX - rho, hi = ST_DMAX + ST_TILE - 1 + rho;
    // the four sides without their corners, from the middle outwards (so that each new cell has placed neighbours on
    // the inner ring and, after the first, on its own side), then the corners
    const int mid = (lo + hi) / 2;
    for (int k = 0; k <= hi - lo; ++k) {
      const int off = (k + 1) / 2 * ((k & 1) ? 1 : -1);  // 0, +1, -1, +2, -2, ...
      const int u = mid + off;
      if (u <= lo || u >= hi) continue;
      if (!place(u, hi) || !place(u, lo) || !place(lo, u) || !place(hi, u)) return false;
    }
    if (!place(lo, lo) || !place(hi, lo) || !place(lo, hi) || !place(hi, hi)) return false;
  }
  // tables + verification
  const int blo = ST_DMAX - D, bhi = ST_DMAX + ST_TILE - 1 + D;
  for (int p = 0; p < ST_CELLS; ++p) {
    row[p] = (int32_t)r0;
    for (int j = 0; j < ST_TABV; ++j) val[(size_t)p * ST_TABV + j] = 0.f;
  }
  *interior = true;
  for (int y = blo; y <= bhi; ++y)
    for (int x = blo; x <= bhi; ++x) {
      const int32_t r = A[x][y];
      const unsigned p = st_cell_off((unsigned)x, (unsigned)y) / 64u;
      if (r < 0) continue;  // a hole: the tile's first row, all zeros (set above)
      row[p] = r;
      if (r >= out_rows) *interior = false;
      if (x == blo || x == bhi || y == blo || y == bhi) continue;  // outermost ring: input only
      if (r >= plan->n_rows) return false;  // a row that a step evaluates has no row of L~
      const int32_t* c = cols + (size_t)r * W;
      const float* v = vals + (size_t)r * W;
      float* o = val + (size_t)p * ST_TABV;
      unsigned seen = 0;
      for (int j = 0; j < W; ++j) {
        if (v[j] == 0.f) continue;
        int d = -1;
        if (c[j] == r) d = 0;
        else {
          const int cell = hget(c[j]);
          if (cell < 0) return false;
          const int dx = cell % S - x, dy = cell / S - y;
          for (int q = 0; q < 8; ++q)
            if (ddx[q] == dx && ddy[q] == dy) d = q + 1;
          if (d < 0) return false;  // a non-zero that is not on one of the eight neighbouring cells
        }
        if (seen & (1u << d)) return false;
        seen |= 1u << d;
        o[d] = v[j];
      }
    }
  return true;
}

// Steps of the busiest workgroup when the strip kernel deals `steps.size()` pairs x N maps the way cheb_strip5_kernel does:
// items q = pair * N + map, a contiguous eighth of them per XCD, dealt to the XCD's workgroups in turn.
static int strip_grid(int num_cu, int64_t n_items) { return (int)std::max<int64_t>(8, std::min<int64_t>(num_cu, (n_items + 7) / 8 * 8)); }
int64_t strip_makespan(const std::vector<int32_t>& steps, int64_t N, int num_cu) {
  const int64_t Q = (int64_t)steps.size() * N;
  const int G = strip_grid(num_cu, Q);
  int64_t worst = 0;
  std::vector<int64_t> load;
  for (int xcd = 0; xcd < 8; ++xcd) {
    const int nslots = (G + 7 - xcd) / 8;
    const int64_t q0 = Q * xcd / 8, q1 = Q * (xcd + 1) / 8;
    if (nslots <= 0 || q1 <= q0) continue;
    load.assign((size_t)nslots, 0);
    for (int64_t q = q0; q < q1; ++q) load[(size_t)((q - q0) % nslots)] += steps[(size_t)(q / N)];
    for (int64_t v : load) worst = std::max(worst, v);
  }
  return worst;
}

struct TileRect { int tx, ty, wt, ht; };  // a rectangle of the tile plane
// The strip rectangles cut into strip pairs (cheb_strip_kernel.h) of segments of at most h rows
static void cut_strip_pairs(const std::vector<TileRect>& take, int D, int h, std::vector<StripPair>& out) {
  out.clear();
  for (const TileRect& r : take) {
    const int X0 = 16 * r.tx, X1 = 16 * (r.tx + r.wt), Y0 = 16 * r.ty, Y1 = 16 * (r.ty + r.ht);
    const int ns = (X1 - X0 + SP_USE - 1) / SP_USE;
    const int H = Y1 - Y0, nseg = (H + h - 1) / h;
    for (int sg = 0; sg < nseg; ++sg) {
      const int ya = Y0 + (int)((int64_t)H * sg / nseg), yb = Y0 + (int)((int64_t)H * (sg + 1) / nseg);
      for (int s0 = 0; s0 < ns; s0 += 2) {
        StripPair p;
        for (int e = 0; e < 2; ++e) {
          const int s = s0 + e;
          if (s < ns) {
            p.x0[e] = X0 + SP_USE * s;
            p.w[e] = std::min(SP_USE, X1 - p.x0[e]);
          } else {
            p.x0[e] = p.x0[0];
            p.w[e] = 0;
          }
        }
        p.y0 = ya;
        p.y1 = yb;
        p.xlo = X0 - D;
        p.xhi = X1 - 1 + D;
        for (int e = 0; e < 2; ++e)  // lane 0 of the strip: D columns left of the first output column, but never past the halo
          p.xs[e] = std::min(p.x0[e] - D, p.xhi + 1 - SP_PX);
        p.ylo = Y0 - D;
        p.yhi = Y1 - 1 + D;
        out.push_back(p);
      }
    }
  }
  // Items of unequal height (ragged masks): tallest first, then dealt over the eight XCD ranges of the kernel (a range is a
  // contiguous eighth of the list), so that every XCD -- and, the kernel dealing a range to its workgroups in turn, every
  // workgroup -- gets its share of tall and short ones.  Equal heights (a full sphere): the order of the cut stays,
  // neighbours in x next to each other.
  bool ragged = false;
  for (const StripPair& p : out) ragged = ragged || (p.y1 - p.y0 != out[0].y1 - out[0].y0);
  if (ragged) {
    std::stable_sort(out.begin(), out.end(), [](const StripPair& a, const StripPair& b) { return a.y1 - a.y0 > b.y1 - b.y0; });
    std::vector<StripPair> dealt;
    dealt.reserve(out.size());
    for (size_t x = 0; x < 8; ++x)
      for (size_t i2 = x; i2 < out.size(); i2 += 8) dealt.push_back(out[i2]);
    out.swap(dealt);
  }
}

constexpr int SMALL_MAP_TILES = 512;  // structured tiles up to which a plan without strips runs them in ONE launch (class-R tiles with tables)
// Strip kernel: which class-R tiles it takes, and in what pieces.  The interior class-R tiles are covered by rectangles (in
// the virtual Morton plane of the tile indices: tile t sits at (compress(t), compress(t >> 1))) of 3 to 5 tile columns and at
// least 4 tile rows; a rectangle is cut into 32-column strips with 24 output columns each, two strips per workgroup item,
// and into row segments sized so that the items fill the CUs evenly.  The other tiles stay with the tile kernels (`rest`).
static void build_strips(const std::vector<int32_t>& r_interior, int D, int num_cu, const PlanOptions& opt,
                         std::vector<StripPair>& pairs, std::vector<int32_t>& rest, int64_t* n_taken, std::vector<int32_t>& steps,
                         std::vector<StripPair>& whole) {  // whole: the same strips uncut along y (input-side strip kernel)
  steps.clear();
  pairs.clear();
  whole.clear();
  rest.clear();
  *n_taken = 0;
  // columns of the tile plane and their vertical runs of class-R tiles
  std::vector<uint64_t> keys(r_interior.size());  // (tx, ty)
  for (size_t i = 0; i < r_interior.size(); ++i) {
    const unsigned t = (unsigned)r_interior[i];
    keys[i] = ((uint64_t)st_compress(t) << 32) | st_compress(t >> 1);
  }
  std::sort(keys.begin(), keys.end());
  struct Run { int tx, y0, y1; bool used; };
  std::vector<Run> runs;
  for (size_t i = 0; i < keys.size();) {
    const int tx = (int)(keys[i] >> 32), y0 = (int)(keys[i] & 0xffffffffu);
    size_t j = i + 1;
    while (j < keys.size() && (int)(keys[j] >> 32) == tx && (int)(keys[j] & 0xffffffffu) == y0 + (int)(j - i)) ++j;
    runs.push_back({tx, y0, y0 + (int)(j - i), false});
    i = j;
  }
  // Groups of 3 (at the end of a stretch: 4 or 5) adjacent columns whose runs share at least 4 rows: one rectangle each, of the
  // shared rows.  (Three tile columns = 48 pixels = one pair of strips; tall rather than wide, the strips run along y.  On a
  // full base pixel every column has the same run and nothing is left over; on a mask the rows a group does not share, and
  // stretches of fewer than 3 columns, stay with the tile kernels.)
  auto overlap = [](int a0, int a1, int b0, int b1, int* o0, int* o1) { *o0 = std::max(a0, b0); *o1 = std::min(a1, b1); return *o1 - *o0; };
  const int min_rows = std::max(4, opt.strip_min_rows);  // (tuning, DSPH_OPT_STRIP_MINROWS: least height of a rectangle, in tiles)
  std::vector<TileRect> take;
  for (size_t i = 0; i < runs.size(); ++i) {
    if (runs[i].used) continue;
    // how many adjacent columns continue this run with at least 4 shared rows (at most 6 looked at)
    std::vector<size_t> chain{i};
    int y0 = runs[i].y0, y1 = runs[i].y1;
    while (chain.size() < 6) {
      const int want = runs[chain.back()].tx + 1;
      size_t best = runs.size();
      int by0 = 0, by1 = 0;
      for (size_t j = chain.back() + 1; j < runs.size() && runs[j].tx <= want; ++j) {
        int o0, o1;
        if (runs[j].tx == want && !runs[j].used && overlap(y0, y1, runs[j].y0, runs[j].y1, &o0, &o1) >= min_rows &&
            (best == runs.size() || o1 - o0 > by1 - by0)) { best = j; by0 = o0; by1 = o1; }
      }
      if (best == runs.size()) break;
      if (chain.size() < 5) { y0 = by0; y1 = by1; }  // (the sixth only says "the stretch goes on")
      chain.push_back(best);
    }
    const int avail = (int)chain.size();
    if (avail < 3 || y1 - y0 < min_rows) continue;  // stays with the tile kernels
    const int w = avail >= 6 ? 3 : std::min(avail, 5);
    // the shared rows of the w columns actually taken
    y0 = runs[chain[0]].y0; y1 = runs[chain[0]].y1;
    for (int c = 1; c < w; ++c) { int o0, o1; overlap(y0, y1, runs[chain[c]].y0, runs[chain[c]].y1, &o0, &o1); y0 = o0; y1 = o1; }
    if (y1 - y0 < min_rows) continue;
    take.push_back({runs[chain[0]].tx, y0, w, y1 - y0});
    *n_taken += (int64_t)w * (y1 - y0);
    for (int c = 0; c < w; ++c) {
      Run& r = runs[chain[c]];
      // what the rectangle leaves of the run: above / below stay as (used) leftovers for the tile kernels
      for (int y = r.y0; y < r.y1; ++y)
        if (y < y0 || y >= y1) rest.push_back((int32_t)st_morton((unsigned)r.tx, (unsigned)y));
      r.used = true;
    }
  }
  for (const Run& r : runs)
    if (!r.used)
      for (int y = r.y0; y < r.y1; ++y) rest.push_back((int32_t)st_morton((unsigned)r.tx, (unsigned)y));
  std::sort(rest.begin(), rest.end());
  if (take.empty()) return;
  // Segment height: every segment pays 2 D + 1 run-in rows, every workgroup should get the same number of steps.  Candidates
  // from the whole rectangle down to 256 rows (measured on the partial sky of BASELINE configs[4], batch 16, strips forced:
  // 23.0 ms with 64-row segments, 21.6 with 128, 21.3 with 256 and 512, 21.6 unsegmented; the tile kernels: 21.8); the one whose busiest workgroup has the fewest steps
  // for ONE map wins -- a batch only evens things out further, items being (pair, map).
  auto steps_of = [&](const std::vector<StripPair>& v, std::vector<int32_t>& st) {
    st.resize(v.size());
    for (size_t i2 = 0; i2 < v.size(); ++i2) st[i2] = (v[i2].y1 - v[i2].y0) + 2 * D + 1;
  };
  const int cand[] = {4096, 2048, 1024, 512, 384, 256};
  int64_t best_span = -1;
  int best_h = 256;
  {
    std::vector<StripPair> trial;
    std::vector<int32_t> st;
    for (int h : cand) {
      cut_strip_pairs(take, D, h, trial);
      steps_of(trial, st);
      const int64_t span = strip_makespan(st, 1, num_cu);
      if (best_span < 0 || span < best_span) { best_span = span; best_h = h; }
    }
  }
  cut_strip_pairs(take, D, best_h, pairs);
  steps_of(pairs, steps);
  cut_strip_pairs(take, D, 1 << 30, whole);
}

// ---- table-addressed quad strips (round 6) ----------------------------------------------------------------------------------
// A candidate tile of the logical grid: its eight neighbour TILES by direction (kDirX / kDirY order: W NW N NE E SE S SW), each
// verified to continue this tile's own 16 x 16 Morton square by a pure translation over the D rows / columns a strip's halo
// reaches into it.  Class R: the neighbours of the virtual Morton plane (what the classification verified).  Class T: read off
// the embedding embed_tile() found and verified (row[] = the row of every plane cell).
struct QCand {
  int32_t tile;
  int32_t nbr[8];
  int32_t tix;       // position in the class-T list (tables), -1 for a class-R tile
  int32_t sheet, u, v;
  bool taken;
  bool barred;       // stays with the tile kernels whatever the rectangles would gain (a cell no rectangle may cover)
};

static bool links_from_table(const int32_t* row, int D, int32_t ntiles, int32_t nbr[8]) {
  for (int d = 0; d < 8; ++d) {
    const int xa = ddx[d] < 0 ? ST_DMAX - D : (ddx[d] == 0 ? ST_DMAX : ST_DMAX + ST_TILE);
    const int xb = ddx[d] < 0 ? ST_DMAX : (ddx[d] == 0 ? ST_DMAX + ST_TILE : ST_DMAX + ST_TILE + D);
    const int ya = ddy[d] < 0 ? ST_DMAX - D : (ddy[d] == 0 ? ST_DMAX : ST_DMAX + ST_TILE);
    const int yb = ddy[d] < 0 ? ST_DMAX : (ddy[d] == 0 ? ST_DMAX + ST_TILE : ST_DMAX + ST_TILE + D);
    int64_t base = -1;
    for (int y = ya; y < yb; ++y)
      for (int x = xa; x < xb; ++x) {
        const int64_t r = row[st_cell_off((unsigned)x, (unsigned)y) / 64u];
        const int64_t b = r - (int64_t)st_morton((unsigned)(x - ST_DMAX) & 15u, (unsigned)(y - ST_DMAX) & 15u);
        if (b < 0 || (b & (FUSED_P - 1)) != 0 || (base >= 0 && b != base)) return false;
        base = b;
      }
    if (base < 0 || base / FUSED_P >= ntiles) return false;
    nbr[d] = (int32_t)(base / FUSED_P);
  }
  return true;
}

// What a rectangle of w x h tiles saves against the tile kernels, in units of 0.1 us of one CU and one map (the constants of
// strips_apply: 18.7 us per tile, 2.8 us per strip step): strips of 56 output columns, 2 D + 1 run-in steps each.
// (the K = 8 strips -- cheb_qstrip8_kernel.h, D = 7 -- have 50 output columns, 16 run-in steps, ~2.6 us a step, against 27.5 us
// per tile on the breadth-first tile kernel with its 7-ring halo)
static int64_t qt_gain(int w, int h, int D) {
  const int use = D == Q8_D ? Q8_USE : QS_PX - 2 * D;
  const int64_t ns = (16 * (int64_t)w + use - 1) / use;
  if (D == Q8_D) return (int64_t)w * h * 275 - ns * (16 * (int64_t)h + Q8_RUNIN) * 26;
  // (a run of rows costs more than its 2 D + 1 run-in steps: two barriers and a waited-for first row before the loop, the step
  // count rounded up to a multiple of three -- measured at the headline map, 254 strips against 216: about 14 steps a run)
  return (int64_t)w * h * 187 - ns * (16 * (int64_t)h + 2 * D + 6) * 28;
}

// Sheets: logical coordinates (sheet, u, v) of every candidate by breadth-first search over the four axis links that both
// ends agree on; returns the number of sheets.
static int32_t assign_sheets(std::vector<QCand>& cands, int32_t ntiles) {
  const int n = (int)cands.size();
  std::vector<int32_t> cand_of((size_t)ntiles, -1);
  for (int i = 0; i < n; ++i) cand_of[(size_t)cands[i].tile] = i;
  auto cand_at = [&](int32_t tile) -> int { return tile >= 0 && tile < ntiles ? cand_of[(size_t)tile] : -1; };
  std::unordered_map<uint64_t, int32_t> at;  // (sheet, u, v) -> candidate
  constexpr int64_t OFF = 1 << 20;
  auto key_of = [&](int32_t sheet, int64_t u, int64_t v) { return ((uint64_t)sheet << 44) | ((uint64_t)(u + OFF) << 22) | (uint64_t)(v + OFF); };
  int32_t nsheets = 0;
  std::vector<int32_t> queue;
  for (int i = 0; i < n; ++i) cands[i].sheet = -1;
  for (int i0 = 0; i0 < n; ++i0) {
    if (cands[i0].sheet >= 0) continue;
    if (nsheets >= (1 << 19)) break;
    const int32_t sh = nsheets++;
    cands[i0].sheet = sh; cands[i0].u = 0; cands[i0].v = 0;
    at[key_of(sh, 0, 0)] = i0;
    queue.assign(1, i0);
    for (size_t h = 0; h < queue.size(); ++h) {
      const QCand a = cands[(size_t)queue[h]];
      for (int d = 0; d < 8; d += 2) {
        const int b = cand_at(a.nbr[d]);
        if (b < 0 || cands[(size_t)b].sheet >= 0 || cands[(size_t)b].nbr[(d + 4) & 7] != a.tile) continue;
        const int64_t u = (int64_t)a.u + ddx[d], v = (int64_t)a.v + ddy[d];
        if (u <= -OFF + 2 || u >= OFF - 2 || v <= -OFF + 2 || v >= OFF - 2) continue;
        const uint64_t k = key_of(sh, u, v);
        if (at.find(k) != at.end()) continue;  // (a sphere unrolled onto the plane meets itself again: the place is taken)
        cands[(size_t)b].sheet = sh; cands[(size_t)b].u = (int32_t)u; cands[(size_t)b].v = (int32_t)v;
        at[k] = b;
        queue.push_back(b);
      }
    }
  }
  return nsheets;
}

// The kernel cuts the tape of all strips' rows into equal pieces, and a piece pays 2 D + 1 run-in steps for every strip that
// begins in it: the greedy extraction leaves the low strips (a few tiles high) at the end of the list, where a piece would
// hold dozens of them (measured at the headline map: the last pieces took 14 % longer than the first, and the forward with
// them).  So the low strips are dealt out evenly between the tall ones, by rows.
static void deal_low_strips(std::vector<QStrip>& strips) {
  std::vector<QStrip> tall, low;
  int64_t rows_tall = 0, rows_low = 0;
  for (const QStrip& q : strips) {
    if (q.y1 - q.y0 >= 256) { tall.push_back(q); rows_tall += q.y1 - q.y0; }
    else { low.push_back(q); rows_low += q.y1 - q.y0; }
  }
  if (!tall.empty() && !low.empty()) {
    strips.clear();
    size_t li = 0;
    int64_t done_tall = 0, done_low = 0;
    for (const QStrip& q : tall) {
      strips.push_back(q);
      done_tall += q.y1 - q.y0;
      while (li < low.size() && done_low * rows_tall < rows_low * done_tall) {
        strips.push_back(low[li]);
        done_low += low[li].y1 - low[li].y0;
        ++li;
      }
    }
    for (; li < low.size(); ++li) strips.push_back(low[li]);
  }
}

// Rectangles of candidate tiles on the logical grid and their strips.  cands: every interior class-R tile and every eligible
// interior class-T tile.  Out: strips (coordinates relative to the rectangle's table: the rectangle's first pixel is (16, 16)),
// the tables, `taken` set in cands.
static void build_qtstrips(std::vector<QCand>& cands, int32_t ntiles, int D, std::vector<QStrip>& strips, std::vector<int32_t>& tab,
                           int64_t* n_taken) {
  strips.clear();
  tab.clear();
  *n_taken = 0;
  const int n = (int)cands.size();
  if (n == 0) return;
  const int32_t nsheets = assign_sheets(cands, ntiles);
  // per sheet: occupancy grid over the bounding box, greedy extraction of the rectangle with the largest gain
  std::vector<std::vector<int32_t>> members((size_t)nsheets);
  for (int i = 0; i < n; ++i)
    if (cands[i].sheet >= 0) members[(size_t)cands[i].sheet].push_back(i);
  for (int32_t sh = 0; sh < nsheets; ++sh) {
    const std::vector<int32_t>& mem = members[(size_t)sh];
    if (mem.size() < 6) continue;
    int u0 = 1 << 30, u1 = -(1 << 30), v0 = 1 << 30, v1 = -(1 << 30);
    for (int32_t i : mem) { u0 = std::min(u0, cands[(size_t)i].u); u1 = std::max(u1, cands[(size_t)i].u); v0 = std::min(v0, cands[(size_t)i].v); v1 = std::max(v1, cands[(size_t)i].v); }
    const int64_t GW = (int64_t)u1 - u0 + 1, GH = (int64_t)v1 - v0 + 1;
    if (GW * GH > (1ll << 26)) continue;  // (a sheet that sprawls: left to the tile kernels)
    std::vector<int32_t> grid((size_t)(GW * GH), -1);  // candidate index, -1 empty, -2 blocked
    for (int32_t i : mem) grid[(size_t)((cands[(size_t)i].v - v0) * GW + (cands[(size_t)i].u - u0))] = cands[(size_t)i].barred ? -2 : i;
    std::vector<int32_t> hgt((size_t)GW);
    std::vector<std::pair<int, int>> stack;  // (start column, height)
    // (every extraction sweeps the sheet once: a budget of sweeps bounds the set-up time on ragged masks -- what is not taken
    // by then stays with the tile kernels)
    for (int64_t sweeps = 0; sweeps * GW * GH < (3ll << 28) && sweeps < 8192; ++sweeps) {
      // the best (gain) rectangle of free cells: histogram of free runs along v, one sweep per row
      int64_t best = 0;
      int bu = 0, bv = 0, bw = 0, bh = 0;
      std::fill(hgt.begin(), hgt.end(), 0);
      for (int64_t y = 0; y < GH; ++y) {
        for (int64_t x = 0; x < GW; ++x) hgt[(size_t)x] = grid[(size_t)(y * GW + x)] >= 0 ? hgt[(size_t)x] + 1 : 0;
        stack.clear();
        for (int64_t x = 0; x <= GW; ++x) {
          const int hx = x < GW ? hgt[(size_t)x] : 0;
          int start = (int)x;
          while (!stack.empty() && stack.back().second > hx) {
            const int s0 = stack.back().first, hh = stack.back().second;
            stack.pop_back();
            const int wmax = (int)x - s0;
            // the widest rectangle of this height, or one a few columns narrower where the last strip would be nearly empty
            for (int w = std::min(wmax, 1000); w >= std::max(1, std::min(wmax, 1000) - 3); --w) {  // (1,000: the kernels keep a tile column in ten bits)
              const int64_t g = qt_gain(w, hh, D);
              if (g > best) { best = g; bu = s0; bv = (int)y - hh + 1; bw = w; bh = hh; }
            }
            start = s0;
          }
          if (hx > 0 && (stack.empty() || stack.back().second < hx)) stack.push_back({start, hx});
        }
      }
      if (best <= 0) break;
      // the table of tile bases: the rectangle and one ring of tiles around it
      const int TW = bw + 2, TH = bh + 2;
      std::vector<int32_t> t((size_t)TW * TH, -1);
      bool good = true;
      auto inside = [&](int i, int j) { return i >= 1 && i <= bw && j >= 1 && j <= bh; };
      for (int j = 1; j <= bh && good; ++j)
        for (int i = 1; i <= bw && good; ++i) {
          const int32_t c = grid[(size_t)((bv + j - 1) * GW + (bu + i - 1))];
          const QCand& q = cands[(size_t)c];
          t[(size_t)j * TW + i] = q.tile;
          for (int d = 0; d < 8 && good; ++d) {
            const int i2 = i + ddx[d], j2 = j + ddy[d];
            int32_t& slot = t[(size_t)j2 * TW + i2];
            if (inside(i2, j2)) {  // the neighbour inside the rectangle must be the tile the grid holds there
              const int32_t c2 = grid[(size_t)((bv + j2 - 1) * GW + (bu + i2 - 1))];
              if (cands[(size_t)c2].tile != q.nbr[d]) good = false;
            } else if (slot < 0) slot = q.nbr[d];
            else if (slot != q.nbr[d]) good = false;  // two tiles of the rectangle name different tiles for one place of the ring
          }
        }
      if (!good) {  // (a seam the sheet's coordinates paper over: these tiles stay with the tile kernels)
        for (int j = 0; j < bh; ++j)
          for (int i = 0; i < bw; ++i) grid[(size_t)((bv + j) * GW + (bu + i))] = -2;
        continue;
      }
      const int32_t toff = (int32_t)tab.size();
      for (int32_t tile : t) tab.push_back(tile < 0 ? 0 : tile * FUSED_P);  // (the four corners of the ring of a 1-wide rectangle ... are never -1: every ring place has a neighbour inside)
      for (int j = 0; j < bh; ++j)
        for (int i = 0; i < bw; ++i) {
          int32_t& c = grid[(size_t)((bv + j) * GW + (bu + i))];
          cands[(size_t)c].taken = true;
          c = -2;
        }
      *n_taken += (int64_t)bw * bh;
      const int X0 = 16, X1 = 16 + 16 * bw, Y0 = 16, Y1 = 16 + 16 * bh;
      // output columns of a strip, and how far left of the first one its lane 0 stands: the kernels take a lane's four pixels
      // for one aligned group of four inside one tile, so both are multiples of four (D = 7: 48 columns behind 8 of lead-in)
      const int use = D == Q8_D ? Q8_USE : QS_PX - 2 * D, lead = D == Q8_D ? 8 : D;
      for (int x0 = X0; x0 < X1; x0 += use) {
        QStrip q{};
        q.x0 = x0; q.w = std::min(use, X1 - x0); q.xs = x0 - lead;
        q.y0 = Y0; q.y1 = Y1;
        q.xlo = X0 - D; q.xhi = X1 - 1 + D; q.ylo = Y0 - D; q.yhi = Y1 - 1 + D;
        q.tab = toff; q.tws = TW;
        strips.push_back(q);
      }
    }
  }
  deal_low_strips(strips);
}

// ---- get_tiles, stage by stage ----------------------------------------------------------------------------------------------
// what every stage reads of the plan
struct Graph {
  const dsph_plan* plan;
  const int32_t* cols;
  const float* vals;
  int W;             // ELL width of the plan
  int64_t out_rows;  // the plan's output rows
  int ntiles;
};

// a list of tiles on the host: the interior ones first
struct HostList {
  std::vector<int32_t> v;
  int n_interior = 0;
};
static HostList joined(std::vector<int32_t> interior, const std::vector<int32_t>& boundary) {
  HostList h;
  h.n_interior = (int)interior.size();
  h.v = std::move(interior);
  h.v.insert(h.v.end(), boundary.begin(), boundary.end());
  return h;
}

// class-T tables on the host: [n] tiles (interior ones first once joined), [n][ST_CELLS] rows, [n][ST_CELLS][ST_TABV] values
struct TTabs {
  std::vector<int32_t> tiles, rows;
  std::vector<float> vals;
  int n_interior = 0;
  void add(int32_t t, const int32_t* row, const float* val) {
    tiles.push_back(t);
    rows.insert(rows.end(), row, row + ST_CELLS);
    vals.insert(vals.end(), val, val + (size_t)ST_CELLS * ST_TABV);
  }
  void add(const TTabs& o, size_t i) { add(o.tiles[i], &o.rows[i * ST_CELLS], &o.vals[i * ST_CELLS * ST_TABV]); }
};
static TTabs joined(TTabs interior, const TTabs& boundary) {
  interior.n_interior = (int)interior.tiles.size();
  for (size_t i = 0; i < boundary.tiles.size(); ++i) interior.add(boundary, i);
  return interior;
}

// embed_tile's result and scratch
struct Embedding {
  std::vector<int32_t> row = std::vector<int32_t>(ST_CELLS), key, slot;
  std::vector<float> val = std::vector<float>((size_t)ST_CELLS * ST_TABV);
  bool interior = false;
  bool run(const Graph& g, int t, int D) {
    return embed_tile(g.plan, g.cols, g.vals, g.W, t, D, g.out_rows, row.data(), val.data(), &interior, key, slot);
  }
};

// the tiles of a plan by class, interior and boundary ones apart
struct Classes {
  std::vector<int32_t> r_in, r_bd;  // class R: the structured kernel
  TTabs t_in, t_bd;                 // class T: the structured kernel with per-tile tables
  std::vector<int32_t> g_in, g_bd;  // class G: the breadth-first tile kernel
};

// the breadth-first tables (layout: cheb_fused_kernel.h) and the scratch of bfs_tile
struct BfsTables {
  std::vector<int32_t> tile_off, ring_end, region;
  std::vector<int64_t> ell_off;
  std::vector<uint16_t> lcols;
  std::vector<float> lvals;
  int rmax = 0, emax = 0;
  int64_t ell_rows = 0;
  std::vector<int32_t> stamp, local, ring, next;
};

// everything upload_tables sends to the device
struct HostTables {
  BfsTables bfs;
  HostList part, r, rrest, qrrest, q8rest, all, nonq;
  TTabs t, qt;
  std::vector<StripPair> pairs, ipairs;
  std::vector<int32_t> patch_rows;  // class-T rows on the K = 5 quad strips and their values by direction (struct_patch_rows)
  std::vector<float> patch_vals;
};

// the direction-ordered copy of L~ and the per-row regularity flags (struct_build_rows), tried once per plan
static void ensure_rows(const dsph_plan* plan, FusedPlan* fp) {
  if (fp->rows_tried) return;
  fp->rows_tried = true;
  if (struct_build_rows(plan, &fp->d_gvals8, &fp->d_gdiag, &fp->d_rowflag) != DSPH_OK) {
    if (fp->d_gvals8) (void)hipFree(fp->d_gvals8);
    if (fp->d_gdiag) (void)hipFree(fp->d_gdiag);
    if (fp->d_rowflag) (void)hipFree(fp->d_rowflag);
    fp->d_gvals8 = fp->d_gdiag = nullptr;
    fp->d_rowflag = nullptr;
  }
}

// Classification: cls[t] bit 0 class R, bit 1 interior (struct_classify_tiles); all zero where the structured kernel is not in
// play.  K = 8 quad strips: which tiles' 7-ring regions are regular squares of the Morton plane (the same row flags, a deeper
// ring; cls8, empty where those strips do not apply).  Every tile still gets its breadth-first tables (other shapes and the
// weight gradient run on them).  On a sharded plan the candidates are the INTERIOR tiles (region inside the rank's own rows):
// they run with the interior part of a forward.
static void classify(const Graph& g, FusedPlan* fp, int D, bool full, std::vector<unsigned char>& cls, std::vector<unsigned char>& cls8) {
  const dsph_plan* plan = g.plan;
  cls.assign((size_t)g.ntiles, 0);
  if (!full && D <= ST_DMAX && plan->opt.use_struct) {
    ensure_rows(plan, fp);
    if (fp->d_rowflag && struct_classify_tiles(plan, fp->d_rowflag, g.ntiles, D, g.out_rows, cls.data()) != DSPH_OK)
      std::fill(cls.begin(), cls.end(), 0);
  }
  if (D == Q8_D && plan->opt.use_struct && plan->opt.strips != 2 && plan->opt.strip_form == 0 && !fp->wide) {
    ensure_rows(plan, fp);
    if (fp->d_rowflag) {
      cls8.assign((size_t)g.ntiles, 0);
      if (struct_classify_tiles(plan, fp->d_rowflag, g.ntiles, D, g.out_rows, cls8.data(), Q8_D) != DSPH_OK) cls8.clear();
    }
  }
}

// Emit a ring so that (local index & 3) == (row id & 3) wherever possible.  On a HEALPix map the low two NEST bits are the
// pixel's (x, y) parity; the recurrence reads the j-th neighbours of four rows with four different parities in one LDS access
// group, and those neighbours then sit in four different bank quarters -- halo rows included, not only the tile's own rows.
// at: local index of the ring's first entry.
static void deal_by_parity(std::vector<int32_t>& ring, size_t at) {
  std::vector<int32_t> bucket[4];
  for (int32_t r : ring) bucket[r & 3].push_back(r);
  size_t head[4] = {0, 0, 0, 0};
  size_t left = ring.size();
  ring.clear();
  while (left > 0) {
    const int want = (int)((at + ring.size()) & 3);
    int take = want;
    if (head[take] >= bucket[take].size()) {  // that parity is used up: take from the fullest
      size_t best = 0;
      for (int q = 0; q < 4; ++q) {
        const size_t rem = bucket[q].size() - head[q];
        if (rem > best) { best = rem; take = q; }
      }
    }
    ring.push_back(bucket[take][head[take]++]);
    --left;
  }
}

// Row i of a tile-local ELL of E rows, stored [slot][row] (lc[j * E + i]); c / v: the row of the plan's ELL.
static void ell_row(const int32_t* c, const float* v, int W, int WT, int i, int E, const int32_t* local, uint16_t* lc, float* lv) {
  for (int j = 0; j < WT; ++j) {
    uint16_t col = (uint16_t)i;
    float val = 0.f;
    if (j < W && v[j] != 0.f) {
      col = (uint16_t)local[c[j]];
      val = v[j];
    }
    lc[(size_t)j * E + i] = col;
    lv[(size_t)j * E + i] = val;
  }
}
// ... for the tiled step (cheb_tstep.hip), which reads slot j of four consecutive rows in one 16-lane LDS access: conflict-free
// when the four neighbours' local indices differ mod 4.  So the slots of a row are dealt by residue: slot j of local row i takes
// a neighbour with (local index & 3) == ((i + j) & 3) while there is one, else one from the fullest residue class (the sum's
// ORDER changes, not its terms).  R: rows of the region.
static void ell_row_wide(const int32_t* c, const float* v, int W, int WT, int i, int E, int R, const int32_t* local, uint16_t* lc,
                         float* lv) {
  std::vector<std::pair<uint16_t, float>> bucket[4];
  for (int j = 0; j < W; ++j)
    if (v[j] != 0.f) bucket[local[c[j]] & 3].push_back({(uint16_t)local[c[j]], v[j]});
  size_t head[4] = {0, 0, 0, 0};
  for (int j = 0; j < WT; ++j) {
    int b = (i + j) & 3;
    if (head[b] >= bucket[b].size()) {
      size_t best = 0;
      int bb = -1;
      for (int q = 0; q < 4; ++q)
        if (bucket[q].size() - head[q] > best) { best = bucket[q].size() - head[q]; bb = q; }
      b = bb;
    }
    uint16_t col = (uint16_t)i;
    float val = 0.f;
    if (b >= 0) {
      col = bucket[b][head[b]].first;
      val = bucket[b][head[b]].second;
      ++head[b];
    } else {
      const int want = (i & ~3) | ((i + j) & 3);  // padding: a row of this quad with the slot's residue (value 0)
      col = (uint16_t)(want < R ? want : i);
    }
    lc[(size_t)j * E + i] = col;
    lv[(size_t)j * E + i] = val;
  }
}

// The breadth-first region of tile t (its own rows, then ring 1 .. D), its ring ends and the tile-local ELL of the rows within
// D - 1 hops, appended to b.  false: the tables cannot be built (a row that must be computed has no ELL row, or the region
// has more rows than the uint16 local columns address).
static bool bfs_tile(const Graph& g, int t, int D, int WT, bool wide, BfsTables& b, bool* inner) {
  const int64_t r0 = (int64_t)t * FUSED_P, r1 = std::min<int64_t>(g.out_rows, r0 + FUSED_P);
  const size_t base = b.region.size();
  b.ring.clear();
  for (int64_t r = r0; r < r1; ++r) {
    b.stamp[r] = t;
    b.local[r] = (int32_t)(r - r0);
    b.ring.push_back((int32_t)r);
    b.region.push_back((int32_t)r);
  }
  int32_t* re = &b.ring_end[(size_t)t * (FUSED_DMAX + 1)];
  re[0] = (int32_t)b.ring.size();
  for (int d = 1; d <= D; ++d) {
    b.next.clear();
    for (int32_t r : b.ring) {
      if (r >= g.plan->n_rows) return false;  // a row that must be computed has no ELL row
      const int32_t* c = g.cols + (size_t)r * g.W;
      const float* v = g.vals + (size_t)r * g.W;
      for (int j = 0; j < g.W; ++j) {
        if (v[j] == 0.f) continue;
        const int32_t cj = c[j];
        if (b.stamp[cj] != t) {
          b.stamp[cj] = t;
          b.next.push_back(cj);
        }
      }
    }
    std::sort(b.next.begin(), b.next.end());
    deal_by_parity(b.next, b.region.size() - base);
    for (int32_t r : b.next) {
      b.local[r] = (int32_t)(b.region.size() - base);
      b.region.push_back(r);
    }
    re[d] = (int32_t)(b.region.size() - base);
    b.ring.swap(b.next);
  }
  for (int d = D + 1; d <= FUSED_DMAX; ++d) re[d] = re[D];
  const int R = re[D], E = re[D - 1];
  *inner = true;
  for (size_t i = base; i < b.region.size() && *inner; ++i) *inner = b.region[i] < g.out_rows;
  if (R > 65535) return false;  // uint16 local columns
  b.rmax = std::max(b.rmax, R);
  b.emax = std::max(b.emax, E);
  const size_t lbase = b.lcols.size();
  b.lcols.resize(lbase + (size_t)E * WT, 0);
  b.lvals.resize(lbase + (size_t)E * WT, 0.f);
  for (int i = 0; i < E; ++i) {
    const int32_t r = b.region[base + i];
    if (r >= g.plan->n_rows) return false;
    const int32_t* c = g.cols + (size_t)r * g.W;
    const float* v = g.vals + (size_t)r * g.W;
    if (wide) ell_row_wide(c, v, g.W, WT, i, E, R, b.local.data(), &b.lcols[lbase], &b.lvals[lbase]);
    else ell_row(c, v, g.W, WT, i, E, b.local.data(), &b.lcols[lbase], &b.lvals[lbase]);
  }
  b.ell_rows += E;
  return true;
}

// Every tile by class: R as classified, T where the class-T tables are tried and embed_tile verifies them, G (breadth-first
// tables) otherwise.  false: the breadth-first tables cannot be built.
static bool sort_tiles(const Graph& g, int D, int WT, bool wide, const std::vector<unsigned char>& cls, bool try_tables,
                       Embedding& em, Classes& c, BfsTables& b) {
  const size_t n_cols = (size_t)g.plan->n_cols;
  b.stamp.assign(n_cols, -1);
  b.local.assign(n_cols, 0);
  b.tile_off.assign((size_t)g.ntiles + 1, 0);
  b.ring_end.assign((size_t)g.ntiles * (FUSED_DMAX + 1), 0);
  b.ell_off.assign((size_t)g.ntiles, 0);
  b.region.reserve((size_t)g.ntiles * 600);
  for (int t = 0; t < g.ntiles; ++t) {
    if (b.region.size() > 0x7fffffffULL - 70000) return false;  // offsets are int32
    b.tile_off[t] = (int32_t)b.region.size();
    b.ell_off[t] = b.ell_rows;
    if (cls[t] & 1) {
      ((cls[t] & 2) ? c.r_in : c.r_bd).push_back(t);
      continue;
    }
    if (try_tables && em.run(g, t, D)) {
      (em.interior ? c.t_in : c.t_bd).add(t, em.row.data(), em.val.data());
      continue;
    }
    bool inner = false;
    if (!bfs_tile(g, t, D, WT, wide, b, &inner)) return false;
    (inner ? c.g_in : c.g_bd).push_back(t);
  }
  b.tile_off[g.ntiles] = (int32_t)b.region.size();
  return true;
}

// Small maps (BASELINE configs[0]: nside 64, 192 tiles -- 48 class R, 120 class T, 24 class G) are bound by launches, not by
// work: every structured tile fits the device at once, and two launches (class R, then class T) take twice as long as one.
// Where the strips take nothing anyway, the class-R tiles get tables too and join the class-T launch.
static void merge_small_map(const Graph& g, int D, int num_cu, Embedding& em, Classes& c) {
  if ((c.r_in.empty() && c.r_bd.empty()) ||
      c.r_in.size() + c.r_bd.size() + c.t_in.tiles.size() + c.t_bd.tiles.size() > (size_t)SMALL_MAP_TILES)
    return;
  int64_t taken = 0;
  if (g.plan->opt.strips != 2) {
    std::vector<StripPair> p0, ip0;
    std::vector<int32_t> rest0, steps0;
    build_strips(c.r_in, D, num_cu, g.plan->opt, p0, rest0, &taken, steps0, ip0);
  }
  if (taken != 0) return;
  std::vector<int32_t> keep_i, keep_b;
  for (int pass = 0; pass < 2; ++pass)
    for (int32_t t : pass == 0 ? c.r_in : c.r_bd) {
      if (em.run(g, t, D)) (pass == 0 ? c.t_in : c.t_bd).add(t, em.row.data(), em.val.data());
      else (pass == 0 ? keep_i : keep_b).push_back(t);
    }
  c.r_in.swap(keep_i);
  c.r_bd.swap(keep_b);
}

// The round-3 strips: rectangles of the interior class-R tiles as strip pairs (cut into row segments) and as input-side pairs
// (uncut), and the class-R tiles they leave to the structured kernel.
static void pair_strips(const Graph& g, int D, int num_cu, bool full, const Classes& c, FusedTiles& ft, HostTables& h) {
  std::vector<int32_t> rest = c.r_in;
  ft.strip_forced = g.plan->opt.strips == 1;
  if (!full && D <= SP_DMAX && g.plan->opt.strips != 2)
    build_strips(c.r_in, D, num_cu, g.plan->opt, h.pairs, rest, &ft.n_strip_tiles, ft.strip_steps, h.ipairs);
  h.rrest = joined(std::move(rest), c.r_bd);
  ft.n_pairs = (int)h.pairs.size();
  ft.h_pairs = h.pairs;
  ft.n_ipairs = (int)h.ipairs.size();
  for (const StripPair& ip : h.ipairs) {
    ft.ipair_h.push_back(ip.y1 - ip.y0);
    ft.ipair_second.push_back(ip.w[1] > 0 ? 1 : 0);
  }
}

// A quad-strip candidate whose neighbours are those of the virtual Morton plane (what the classification verified)
static QCand morton_cand(int32_t t, int ntiles) {
  QCand c{};
  c.tile = t; c.tix = -1; c.taken = false;
  const int tx = (int)st_compress((unsigned)t), ty = (int)st_compress((unsigned)t >> 1);
  for (int d = 0; d < 8; ++d) {
    const int nx = tx + ddx[d], ny = ty + ddy[d];
    const int64_t nt = nx < 0 || ny < 0 ? -1 : (int64_t)st_morton((unsigned)nx, (unsigned)ny);
    c.nbr[d] = nt >= 0 && nt < ntiles ? (int32_t)nt : -1;
  }
  return c;
}

// The K = 5 quad strips: rectangles on the logical tile grid, addressed through tables (build_qtstrips) -- every interior
// class-R tile and every interior class-T tile whose eight neighbour tiles are pure translations.  Out: the strips, the
// structured kernel's rest lists (qrrest, qt) and the patch rows of the class-T tiles on the strips.
static void quad_strips5(const Graph& g, int D, const Classes& c, FusedTiles& ft, HostTables& h) {
  std::vector<QCand> cands;
  cands.reserve(c.r_in.size() + c.t_in.tiles.size());
  for (int32_t t : c.r_in) cands.push_back(morton_cand(t, g.ntiles));
  const size_t n_rc = cands.size();
  // The kernel does not clamp a row to the strip's halo (cheb_qstrip_kernel.h, "rows need no clamp"): past the halo it reads
  // rows of the table's ring tiles that feed nothing -- rows that must exist.  The one tile whose rows may not is the map's
  // last, incomplete one: no tile beside it is a candidate, so it is in no rectangle's ring.
  const int32_t ragged = g.out_rows % FUSED_P != 0 ? g.ntiles - 1 : -1;
  auto beside_ragged = [&](const QCand& q) {
    if (ragged < 0) return false;
    if (q.tile == ragged) return true;
    for (int d = 0; d < 8; ++d)
      if (q.nbr[d] == ragged) return true;
    return false;
  };
  for (size_t i = 0; i < c.t_in.tiles.size(); ++i) {
    QCand q{};
    q.tile = c.t_in.tiles[i]; q.tix = (int32_t)i; q.taken = false;
    if (links_from_table(&c.t_in.rows[i * ST_CELLS], D, g.ntiles, q.nbr)) cands.push_back(q);
  }
  for (QCand& q : cands) q.barred = beside_ragged(q);
  build_qtstrips(cands, g.ntiles, D, ft.q5.h_strips, ft.q5.h_tab, &ft.q5.n_tiles);
  std::vector<int32_t> r_rest;
  std::vector<unsigned char> t_taken(c.t_in.tiles.size(), 0);
  for (size_t i = 0; i < cands.size(); ++i) {
    if (i < n_rc) { if (!cands[i].taken) r_rest.push_back(cands[i].tile); }  // (r_in is sorted; cands keeps its order)
    else if (cands[i].taken) t_taken[(size_t)cands[i].tix] = 1;
  }
  h.qrrest = joined(std::move(r_rest), c.r_bd);
  TTabs t_rest;
  for (size_t i = 0; i < c.t_in.tiles.size(); ++i) {
    if (!t_taken[i]) {
      t_rest.add(c.t_in, i);
      continue;
    }
    // a class-T tile on the strips: the strips read L~ by direction from gvals8 / gdiag, which the row pass filled from
    // the VIRTUAL Morton plane (a neighbour beyond a base-pixel border has no direction there and was dropped).  The
    // tile's verified embedding has every evaluated row's values by direction: written over the rows' entries (no other
    // kernel reads them for rows that are irregular in the virtual plane; for regular rows the two agree).
    const int blo = ST_DMAX - D + 1, bhi = ST_DMAX + ST_TILE - 1 + D - 1;  // rings 0 .. D-1
    for (int y = blo; y <= bhi; ++y)
      for (int x = blo; x <= bhi; ++x) {
        const size_t cell = i * ST_CELLS + st_cell_off((unsigned)x, (unsigned)y) / 64u;
        h.patch_rows.push_back(c.t_in.rows[cell]);
        h.patch_vals.insert(h.patch_vals.end(), c.t_in.vals.begin() + cell * ST_TABV, c.t_in.vals.begin() + cell * ST_TABV + 9);
      }
  }
  h.qt = joined(std::move(t_rest), c.t_bd);
}

// K = 8: rectangles of the depth-7 regular tiles (virtual Morton neighbours: what the classification verified), and the tiles
// of `part` they leave to the breadth-first tile kernel (interior ones first, like part).
static void quad_strips8(const Graph& g, int D, const std::vector<unsigned char>& cls8, FusedTiles& ft, HostTables& h) {
  std::vector<QCand> cands;
  for (int32_t t = 0; t < g.ntiles; ++t)
    if ((cls8[(size_t)t] & 3) == 3) cands.push_back(morton_cand(t, g.ntiles));
  build_qtstrips(cands, g.ntiles, D, ft.q8.h_strips, ft.q8.h_tab, &ft.q8.n_tiles);
  std::vector<unsigned char> took((size_t)g.ntiles, 0);
  for (const QCand& q : cands)
    if (q.taken) took[(size_t)q.tile] = 1;
  std::vector<int32_t> rest[2];
  for (size_t i = 0; i < h.part.v.size(); ++i)
    if (!took[(size_t)h.part.v[i]]) rest[i < (size_t)h.part.n_interior ? 0 : 1].push_back(h.part.v[i]);
  h.q8rest = joined(std::move(rest[0]), rest[1]);
}

static std::vector<int32_t> cat(std::initializer_list<const std::vector<int32_t>*> lists) {
  std::vector<int32_t> v;
  for (const std::vector<int32_t>* l : lists) v.insert(v.end(), l->begin(), l->end());
  return v;
}

// every tile whatever its class (all: interior ones first), and every tile the K = 5 quad strips leave over (nonq; without
// quad strips the list is not used: the complement of nothing)
static void complements(const Classes& c, const FusedTiles& ft, HostTables& h) {
  h.all = joined(cat({&c.r_in, &c.t_in.tiles, &c.g_in}), cat({&c.r_bd, &c.t_bd.tiles, &c.g_bd}));
  h.nonq.v = ft.q5.n_tiles == 0 ? cat({&c.r_in, &c.r_bd, &c.t_in.tiles, &c.t_bd.tiles, &h.part.v}) : cat({&h.qrrest.v, &h.qt.tiles, &h.part.v});
}

// One device array per host list.  An empty list uploads one zero element (the kernels may read a list's first entry).
template <class T> static bool upload(FusedTiles& ft, T*& dst, std::vector<T>& v) {
  if (v.empty()) v.emplace_back();
  void* p = nullptr;
  if (hipMalloc(&p, v.size() * sizeof(T)) != hipSuccess) return false;
  ft.dev.push_back(p);
  dst = static_cast<T*>(p);
  return hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess;
}
static bool upload(FusedTiles& ft, TileList& dst, HostList& h) {
  dst.n = (int)h.v.size();
  dst.n_interior = h.n_interior;
  return upload(ft, dst.d, h.v);
}
static bool upload(FusedTiles& ft, TileTables& dst, TTabs& h) {
  dst.tiles.n = (int)h.tiles.size();
  dst.tiles.n_interior = h.n_interior;
  return upload(ft, dst.tiles.d, h.tiles) && upload(ft, dst.d_row, h.rows) && upload(ft, dst.d_vals, h.vals);
}
static bool upload(FusedTiles& ft, QStripSet& s) {
  std::vector<QStrip> strips = s.h_strips;
  std::vector<int32_t> prefix(1, 0), tab = s.h_tab;
  for (const QStrip& q : strips) prefix.push_back(prefix.back() + (q.y1 - q.y0));
  // the strips' places in the packed image of L~ (K = 5): rows ylo - 1 .. yhi + 6 each, back to back in list order
  int64_t img_rows = 0;
  for (size_t i = 0; i < strips.size(); ++i) {
    if (img_rows + qstrip_cimage_rows(strips[i]) > INT32_MAX) { img_rows = 0; break; }  // (no image: the kernel gathers)
    strips[i].img = s.h_strips[i].img = (int32_t)img_rows;
    img_rows += qstrip_cimage_rows(strips[i]);
  }
  s.cimg_rows = img_rows;
  s.n = (int)strips.size();
  s.tape_rows = prefix.back();
  tab.resize(tab.size() + 8, 0);  // (a lane's five tile columns are read by scalar loads from the strip's first column on: readable past the end)
  return upload(ft, s.d_strips, strips) && upload(ft, s.d_prefix, prefix) && upload(ft, s.d_tab, tab);
}
static bool upload_tables(FusedTiles& ft, HostTables& h) {
  BfsTables& b = h.bfs;
  return upload(ft, ft.t, h.t) && upload(ft, ft.d_tile_off, b.tile_off) && upload(ft, ft.d_ring_end, b.ring_end) &&
         upload(ft, ft.d_ell_off, b.ell_off) && upload(ft, ft.d_region, b.region) && upload(ft, ft.d_lcols, b.lcols) &&
         upload(ft, ft.d_lvals, b.lvals) && upload(ft, ft.part, h.part) && upload(ft, ft.r, h.r) && upload(ft, ft.rrest, h.rrest) &&
         upload(ft, ft.nonq, h.nonq) && upload(ft, ft.all, h.all) && upload(ft, ft.d_pairs, h.pairs) && upload(ft, ft.q5) &&
         upload(ft, ft.q8) && upload(ft, ft.q8rest, h.q8rest) && upload(ft, ft.qrrest, h.qrrest) && upload(ft, ft.qt, h.qt) &&
         upload(ft, ft.d_ipairs, h.ipairs);
}

// The tables of depth D into ft (ft.D and ft.width set); false: the plan has none.
static bool build_tiles(const dsph_plan* plan, FusedPlan* fp, int D, bool full, FusedTiles& ft) {
  const int64_t out_rows = plan->levels.empty() ? plan->n_rows : plan->levels[0];
  const int64_t nt64 = (out_rows + FUSED_P - 1) / FUSED_P;
  if (D < 1 || D > FUSED_DMAX || nt64 > (1 << 30)) return false;
  const Graph g{plan, fp->h_cols.data(), fp->h_vals.data(), plan->width, out_rows, (int)nt64};
  std::vector<unsigned char> cls, cls8;
  classify(g, fp, D, full, cls, cls8);
  // class-T candidates: whatever the classification left over, when the structured kernel is in play at all
  const bool try_tables = !full && D <= ST_DMAX && plan->opt.use_struct && plan->opt.use_tables && fp->d_rowflag != nullptr;
  Embedding em;
  Classes c;
  HostTables h;
  if (!sort_tiles(g, D, ft.width, fp->wide, cls, try_tables, em, c, h.bfs)) return false;
  ft.ntiles = g.ntiles;
  ft.rmax = std::max((h.bfs.rmax + 15) / 16 * 16, FUSED_P);
  ft.emax = h.bfs.emax;
  if (try_tables && D <= SP_DMAX) merge_small_map(g, D, fp->num_cu, em, c);
  h.part = joined(c.g_in, c.g_bd);
  pair_strips(g, D, fp->num_cu, full, c, ft, h);
  if (!full && D == QS_D && plan->opt.strips != 2 && plan->opt.strip_form == 0 && fp->d_gvals8 != nullptr)
    quad_strips5(g, D, c, ft, h);
  if (!cls8.empty()) quad_strips8(g, D, cls8, ft, h);
  complements(c, ft, h);
  h.r = joined(c.r_in, c.r_bd);
  h.t = joined(c.t_in, c.t_bd);
  bool good = upload_tables(ft, h);
  if (good && !h.patch_rows.empty())
    good = struct_patch_rows(plan, fp->d_gvals8, fp->d_gdiag, h.patch_rows.data(), h.patch_vals.data(), (int64_t)h.patch_rows.size()) == DSPH_OK;
  if (!good) {
    ft.release();
    ft.D = D;
  }
  return good;
}

const FusedTiles& get_tiles(const dsph_plan* plan, int D, bool full) {
  FusedPlan* fp = plan->fused;
  std::lock_guard<std::mutex> lock(fp->mu);
  DeviceGuard guard(plan->device);  // tables live on the plan's device, whatever the caller's current one is
  const int key = 2 * D + (full ? 1 : 0);
  auto it = fp->by_depth.find(key);
  if (it != fp->by_depth.end()) return it->second;
  // the ELL arrays are gone, or a wide graph (which has the tiled step's tables and nothing else): report "not tileable"
  // without caching anything
  static const FusedTiles none;
  if (fp->host_released || (fp->wide && !(D == 1 && full))) return none;
  FusedTiles& ft = fp->by_depth[key];
  ft.D = D;
  ft.width = fp->wide ? tstep_width(plan->width) : template_width(plan->width);
  ft.ok = build_tiles(plan, fp, D, full, ft);
  return ft;
}

// ---- queries behind the C ABI ------------------------------------------------------------------------------------------------
// tiles of the K-term forward by kernel: class R (structured-tile kernel) and class G (BFS-tile kernel)
bool fused_tile_counts(const dsph_plan* plan, int32_t K, int64_t* n_struct, int64_t* n_bfs) {
  if (!plan->fused || K < 2 || K - 1 > FUSED_DMAX) return false;
  const FusedTiles& ft = get_tiles(plan, K - 1, false);
  if (!ft.ok) return false;
  *n_struct = ft.r.n + ft.t.tiles.n;
  *n_bfs = ft.part.n;
  return true;
}

// the quad strips a strip record of the K-term tables describes; nullptr: the strip pairs
static const QStripSet* record_strips(const dsph_plan* plan, const FusedTiles& ft, int32_t K) {
  const QStripSet* s = K == 5 ? &ft.q5 : (K == Q8_K ? &ft.q8 : nullptr);
  return plan->opt.strip_form == 0 && s && !s->h_strips.empty() ? s : nullptr;
}

// the strip pairs of the K-term tables, 12 int32 each: x0[2], w[2], xs[2], y0, y1, xlo, xhi, ylo, yhi (StripPair); returns how
// many there are (also when cap is smaller), -1 when the plan has no fused tables for this K
int64_t fused_strip_pairs(const dsph_plan* plan, int32_t K, int32_t* out, int64_t cap) {
  if (!plan->fused || K < 2 || K - 1 > FUSED_DMAX) return -1;
  const FusedTiles& ft = get_tiles(plan, K - 1, false);
  if (!ft.ok) return -1;
  static_assert(sizeof(StripPair) == 12 * sizeof(int32_t), "StripPair is twelve int32");
  if (const QStripSet* s = record_strips(plan, ft, K)) {  // the quad strips, in the same record: one strip, the second empty
    const int64_t n = (int64_t)s->h_strips.size();
    for (int64_t i = 0; i < n && i < cap; ++i) {
      const QStrip& q = s->h_strips[(size_t)i];
      const int32_t rec[12] = {q.x0, q.x0, q.w, 0, q.xs, q.xs, q.y0, q.y1, q.xlo, q.xhi, q.ylo, q.yhi};
      memcpy(out + 12 * i, rec, sizeof(rec));
    }
    return n;
  }
  const int64_t n = (int64_t)ft.h_pairs.size();
  for (int64_t i = 0; i < n && i < cap; ++i) memcpy(out + 12 * i, &ft.h_pairs[(size_t)i], sizeof(StripPair));
  return n;
}

// rows of n pixels of strip record `strip` (dsph_plan_strip_rows): through the rectangle's table for the quad strips, the
// virtual Z-order plane for the strip pairs; -1 when there is no such record
int64_t fused_strip_rows(const dsph_plan* plan, int32_t K, int64_t strip, int64_t n, const int32_t* xy, int64_t* rows) {
  if (!plan->fused || K < 2 || K - 1 > FUSED_DMAX) return -1;
  const FusedTiles& ft = get_tiles(plan, K - 1, false);
  if (!ft.ok || strip < 0) return -1;
  if (const QStripSet* s = record_strips(plan, ft, K)) {
    if (strip >= (int64_t)s->h_strips.size()) return -1;
    const QStrip& q = s->h_strips[(size_t)strip];
    // (K = 5: the kernel steps a row's bits without clamping it to the halo -- a run of steps reads rows ylo - 1 .. yhi + 6 of
    // the table's ring tiles, beyond the halo for nothing: they are answered as the kernel reads them)
    const int ya = K == 5 ? q.ylo - 1 : q.ylo, yb = K == 5 ? q.yhi + 6 : q.yhi;
    for (int64_t i = 0; i < n; ++i) {
      const int x = std::min(std::max(xy[2 * i], q.xlo), q.xhi), y = std::min(std::max(xy[2 * i + 1], ya), yb);
      rows[i] = (int64_t)s->h_tab[(size_t)(q.tab + (y >> 4) * q.tws + (x >> 4))] + (int64_t)st_morton((unsigned)x & 15u, (unsigned)y & 15u);
    }
    return n;
  }
  if (strip >= (int64_t)ft.h_pairs.size()) return -1;
  for (int64_t i = 0; i < n; ++i) rows[i] = (int64_t)st_morton((unsigned)xy[2 * i], (unsigned)xy[2 * i + 1]);
  return n;
}

// the image rows of strip record `strip` of the K = 5 quad strips (dsph_plan_strip_image), copied to the host: returns the
// floats of the strip's rows (also when cap is smaller: nothing is copied then), -1 when there is no image
int64_t fused_strip_image(const dsph_plan* plan, int32_t basis, int64_t strip, float* out, int64_t cap) {
  if (!plan->fused) return -1;
  const FusedTiles& ft = get_tiles(plan, QS_D, false);
  const QStripSet* s = ft.ok ? record_strips(plan, ft, 5) : nullptr;
  if (!s || strip < 0 || strip >= (int64_t)s->h_strips.size()) return -1;
  const float* img = qstrip_cimage(plan, ft, basis == DSPH_BASIS_CHEBYSHEV, nullptr);
  if (!img) return -1;
  const QStrip& q = s->h_strips[(size_t)strip];
  const int64_t n = qstrip_cimage_rows(q) * (QS_CROWB / 4);
  if (q.img < 0 || (int64_t)q.img + qstrip_cimage_rows(q) > s->cimg_rows) return -1;
  if (n <= cap && hipMemcpy(out, img + (int64_t)q.img * (QS_CROWB / 4), (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return n;
}

// how a quad-strip forward of N maps on the K = 5 tables cuts its work (qstrip_split)
bool fused_strip_split(const dsph_plan* plan, int64_t N, int32_t* grid, int32_t* pieces, int32_t* wg_per_piece, int64_t* tape_rows) {
  if (!plan->fused || N < 1) return false;
  const FusedTiles& ft = get_tiles(plan, QS_D, false);
  if (!ft.ok || ft.q5.n == 0) return false;
  int g = 0, p = 0, w = 0;
  (void)qstrip_split(plan->fused->num_cu, ft.q5.tape_rows, N, ft.q5.tape_rows / std::max(1, ft.q5.n), &g, &p, &w);
  *grid = g; *pieces = p; *wg_per_piece = w; *tape_rows = ft.q5.tape_rows;
  return true;
}

// L~ equal to its transpose, entry for entry (to fp32 rounding): the product rule the quad-strip weight gradient stands on
// moves T_j from x to dy.
bool fused_symmetric(const dsph_plan* plan) {
  FusedPlan* fp = plan->fused;
  std::lock_guard<std::mutex> lock(fp->mu);
  if (fp->symmetric >= 0) return fp->symmetric == 1;
  if (fp->host_released || plan->n_rows != plan->n_cols) return false;  // (not cached: unknown, or not a square operator)
  const int W = plan->width;
  const int64_t n = plan->n_rows;
  const int32_t* cols = fp->h_cols.data();
  const float* vals = fp->h_vals.data();
  bool sym = true;
  for (int64_t r = 0; r < n && sym; ++r)
    for (int j = 0; j < W; ++j) {
      const int64_t c = cols[r * W + j];
      const float v = vals[r * W + j];
      if (v == 0.f || c == r) continue;  // (padding entries carry zeros)
      if (c < 0 || c >= n) { sym = false; break; }
      // the entry (c, r) must hold the same value (every off-diagonal entry is checked from its own side)
      float back = 0.f;
      for (int i = 0; i < W; ++i)
        if (cols[c * W + i] == r) back += vals[c * W + i];
      // (to the last bits of fp32: a normalised Laplacian D^-1/2 A D^-1/2 evaluated in float64 and rounded may differ by one
      // unit in the last place between (r, c) and (c, r); that moves dW by 1e-7 of itself, far below the arithmetic's 4e-6)
      if (fabsf(back - v) > 2.4e-7f * fmaxf(fabsf(back), fabsf(v))) { sym = false; break; }
    }
  fp->symmetric = sym ? 1 : 0;
  return sym;
}

}  // namespace dsph
