// The tile tables of a plan (cheb_tiles.hip builds them, cheb_fused.hip launches on them): which kernel takes which 16 x 16
// tile, the breadth-first regions of the tiles no structured kernel takes, and the strip rectangles.
#pragma once

#include <map>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "cheb_fused_kernel.h"
#include "cheb_qstrip8_kernel.h"
#include "cheb_qstrip_kernel.h"
#include "cheb_strip_kernel.h"
#include "cheb_struct_kernel.h"

namespace dsph {

// A device list of tiles: the interior ones first (their whole region lies in the plan's output rows -- on a sharded plan they
// need no halo row of another rank), then the boundary ones.  part: 0 every tile, 1 the interior ones, 2 the boundary ones.
struct TileList {
  int32_t* d = nullptr;
  int n = 0, n_interior = 0;
  const int32_t* ptr(int part) const { return part == 2 ? d + n_interior : d; }
  int count(int part) const { return part == 0 ? n : (part == 1 ? n_interior : n - n_interior); }
};

// Class-T tiles (structured kernel with per-tile tables, embed_tile): the tiles, the row of every plane cell ([n][ST_CELLS]) and
// the diagonal + eight directions of L~ per cell in the tile's frame ([n][ST_CELLS][ST_TABV]); a part offsets all three.
struct TileTables {
  TileList tiles;
  int32_t* d_row = nullptr;
  float* d_vals = nullptr;
  size_t first(int part) const { return part == 2 ? (size_t)tiles.n_interior : 0; }
  const int32_t* rows(int part) const { return d_row + first(part) * ST_CELLS; }
  const float* vals(int part) const { return d_vals + first(part) * ST_CELLS * ST_TABV; }
};

// Quad strips (cheb_qstrip_kernel.h, K = 5; cheb_qstrip8_kernel.h, K = 8): rectangles on the logical tile grid cut into strips,
// uncut along y (the kernel cuts the tape of their rows evenly over its workgroups) and addressed through tables of tile bases
// (build_qtstrips): a strip looks its rows up as tab[tile row][tile column] + morton(x & 15, y & 15).
struct QStripSet {
  QStrip* d_strips = nullptr;
  int32_t* d_prefix = nullptr;    // [n + 1] rows before each strip
  int32_t* d_tab = nullptr;       // tile-base tables of all rectangles, back to back (row numbers)
  int n = 0;
  int64_t tape_rows = 0;
  int64_t n_tiles = 0;            // tiles the strips take
  std::vector<QStrip> h_strips;   // host copies (dsph_plan_strip_pairs / _rows: what the seam tests read)
  std::vector<int32_t> h_tab;
  // K = 5: the packed image of L~ (cheb_qstrip.hip, qstrip_cimage_kernel; QStrip::img is a strip's first row of it), one per basis
  // ([0] as it stands: monomial, [1] doubled: Chebyshev), built by the first forward of the basis that finds none (qstrip_cimage:
  // never inside a stream capture) or by dsph_plan_prepare (the Chebyshev one), freed with the tables and when
  // DSPH_OPT_QSTRIP_IMAGE changes.  2,304 bytes per row: cimg_rows x 2,304 per basis.  Under FusedPlan::mu.
  mutable float* d_cimg[2] = {nullptr, nullptr};
  mutable bool cimg_failed = false;  // an allocation failed: not tried again on these tables
  int64_t cimg_rows = 0;
};

struct FusedTiles {
  int D = 0;
  int width = 0;     // ELL width of the tile-local table (template width, >= plan width)
  int ntiles = 0;
  int rmax = 0;      // largest region (rows), rounded up to a multiple of 16, >= FUSED_P
  int emax = 0;      // largest number of rows that carry an ELL row
  bool ok = false;
  // breadth-first tables (cheb_fused_kernel.h): region_rows, ring ends and tile-local ELL of every tile of `part`
  int32_t* d_tile_off = nullptr;
  int32_t* d_ring_end = nullptr;   // [ntiles][FUSED_DMAX + 1]
  int64_t* d_ell_off = nullptr;    // [ntiles] in rows
  int32_t* d_region = nullptr;
  uint16_t* d_lcols = nullptr;
  float* d_lvals = nullptr;
  TileList part;     // the tiles of the BFS-tile kernel: all tiles of a full table, the class-G tiles otherwise
  TileList r;        // class-R tiles (cheb_struct_kernel.h); empty in a full table
  TileTables t;      // class-T tiles
  // strip kernel (cheb_strip_kernel.h): rectangles of interior class-R tiles cut into strip pairs, and the class-R tiles they
  // leave over.  Built next to `r`; which of the two sets a forward uses depends on its shape.
  StripPair* d_pairs = nullptr;
  int n_pairs = 0;
  int64_t n_strip_tiles = 0;
  std::vector<int32_t> strip_steps;        // per pair, in list order: rows + run-in = strip steps of one map
  std::vector<StripPair> h_pairs;          // host copy of d_pairs (dsph_plan_strip_pairs: what the seam tests read)
  mutable std::map<int64_t, int64_t> strip_span;  // batch N -> steps of the busiest workgroup (strip_makespan; under FusedPlan::mu)
  bool strip_forced = false;               // DSPH_OPT_STRIPS = 1 when the tables were built: the cost gate is off
  TileList rrest;
  // K = 5 quad strips: class-R tiles and the class-T tiles whose eight neighbour tiles continue the pixel grid by a pure
  // translation (base-pixel borders between an equatorial and a polar face, superpixel borders of a compacted partial-sky map);
  // what they leave to the structured kernel: class-R tiles and class-T tiles with their tables
  QStripSet q5;
  TileList qrrest;
  TileTables qt;
  // K = 8 quad strips (the tables of depth 7 only): rectangles of the tiles whose 7-ring region is a regular square of the
  // Morton plane, and the tiles they leave to the breadth-first tile kernel (in the order of `part`)
  QStripSet q8;
  TileList q8rest;
  // input-side strip kernel (cheb_istrip_kernel.h): the same rectangles, uncut along y (the kernel cuts every strip into the
  // number of row segments that istrip_segments picks for the batch)
  StripPair* d_ipairs = nullptr;
  int n_ipairs = 0;
  std::vector<int32_t> ipair_h;             // rows of every pair
  std::vector<unsigned char> ipair_second;  // whether its second strip exists
  mutable std::map<int64_t, int> iseg;      // 2 * batch N + narrow -> row segments per strip (under FusedPlan::mu)
  // every tile of the plan: what a two-part launch with a deferred activation finishes per part (launch_struct_act_tiles)
  TileList all;
  // every tile the quad strips leave over, whatever its class (class R rest, T, G): what the BFS-tile kernel's weight-gradient
  // mode runs next to the quad-strip weight gradient (cheb_qwgrad.hip)
  TileList nonq;
  // every device allocation above (cheb_tiles.hip, upload), freed together: release() frees them and empties the tables
  std::vector<void*> dev;
  void release();
};

struct FusedPlan {
  std::vector<int32_t> h_cols;  // host copy of the ELL (needed to build tiles for a new K)
  std::vector<float> h_vals;
  std::mutex mu;
  std::map<int, FusedTiles> by_depth;  // key: 2 * depth + (1: BFS tables of every tile, 0: of the class-G tiles only)
  int num_cu = 256;
  // direction-ordered copy of L~ and the per-row regularity flags (cheb_struct.hip), built on first use
  float* d_gvals8 = nullptr;
  float* d_gdiag = nullptr;
  unsigned char* d_rowflag = nullptr;
  bool rows_tried = false;
  bool host_released = false;  // DSPH_PREPARE_RELEASE_HOST: no tables for further depths
  int symmetric = -1;          // L~ == L~^T entry for entry (fused_symmetric; -1: not looked at yet)
  bool wide = false;           // ELL wider than the fused kernels' templates: only the depth-1 tables of the tiled step exist
  // The BFS-tile launch of a forward writes tiles of y that the structured launches do not touch: it runs on this side stream,
  // forked from and joined back into the caller's stream by the two events (a few dozen face-corner tiles would otherwise
  // hold the whole device for the latency of one tile: 14 of the 44 us of BASELINE configs[0], 57 of 544 us of configs[1]).
  // Created by dsph_plan_prepare on plans whose tables call for a fork (side_stream_ready) -- a prepared forward allocates
  // nothing; fork_mu keeps two host threads that share a plan from interleaving their record / wait pairs.  Capturable: the side stream joins the capture through the fork event and leaves it at the join.
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  bool side_failed = false;
  std::mutex fork_mu;
  // DSPH_FWD_KEEP_WEIGHTS: the caller vouches for the weight VALUES; WHICH images a workspace block holds is the library's
  // own business -- it depends on per-call choices (strips or tiles by the batch, maps packed or not) the caller cannot see.
  // Per workspace block: the shape key the images were packed for and the set of images packed since (IMG_* bits).  A kept
  // call packs what the set lacks; a call that does not keep starts an empty set.
  struct Images { uint64_t key = 0; uint32_t mask = 0; };
  std::mutex img_mu;
  std::unordered_map<const void*, Images> images;
};

// The tables of depth D, built and uploaded on first use; returns a reference to the cached entry (ok: the fused kernels can
// run on them).  full: BFS tables of every tile (planes / weight-gradient modes of the BFS kernel); otherwise the tiles are
// first classified and only the class-G ones (not a plain 2-D stencil square) get BFS tables.
const FusedTiles& get_tiles(const dsph_plan* plan, int D, bool full = false);
// The packed image of L~ of the K = 5 quad strips for a basis, built on first use; nullptr: the option says off, the stream is
// being captured and there is none yet, or there is no memory for it (the kernel then gathers the rows itself: same result).
const float* qstrip_cimage(const dsph_plan* plan, const FusedTiles& ft, bool cheb, hipStream_t stream);
// L~ equal to its transpose, entry for entry (to fp32 rounding)
bool fused_symmetric(const dsph_plan* plan);
// steps of the busiest workgroup of the strip kernel for `steps` (one entry per pair) x N maps
int64_t strip_makespan(const std::vector<int32_t>& steps, int64_t N, int num_cu);

}  // namespace dsph
