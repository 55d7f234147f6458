// Single-launch fused Chebyshev forward: the K planes never leave the compute unit.
//
// Replaces the whole of Chebyshev.call (reference gnn_layers.py:131-150): the reference
// materialises K planes of size |x| in memory (tf.stack) and re-lays them out twice; here a
// workgroup owns a tile of P consecutive rows (NEST order: a 16x16 pixel square on a HEALPix
// map), loads the tile plus its (K-1)-hop halo into LDS one 16-channel slice at a time, runs the
// three-term recurrence in LDS on a region that shrinks by one ring per step, and feeds every
// plane T_k straight into MFMA accumulators that stay in registers until y is written once.
//
// The decomposition is generic: rings come from a breadth-first search over the ELL pattern, so
// k-NN graphs, partial-sky graphs, sharded plans with halo rows and arbitrary sparse matrices all
// take the same path; a graph whose halo does not fit in LDS simply reports "not tileable" and
// the caller falls back to the unfused kernels.
//
// This file is the host side of a call: which kernel takes which tiles (Route, make_route), where the packed weight images
// of a block lie in the workspace (WeightImages), and the three launches built on the two -- the forward of one 64-column
// block, the planes mode and the weight-gradient mode of the BFS-tile kernel.  The tile tables and their lists are described
// in cheb_tiles.h (cheb_tiles.hip builds them), the kernels' LDS and register layouts in the *_kernel.h files.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "cheb_istrip_kernel.h"
#include "cheb_tiles.h"

namespace dsph {

void fused_images_begin(const dsph_plan* plan, const void* ws, uint64_t key, bool keep) {
  FusedPlan* fp = plan->fused;
  if (!fp || !ws) return;
  std::lock_guard<std::mutex> lock(fp->img_mu);
  if (fp->images.size() > 16384 && fp->images.find(ws) == fp->images.end()) fp->images.clear();  // (forgetting only costs a re-pack)
  FusedPlan::Images& im = fp->images[ws];
  if (!keep || im.key != key) { im.key = key; im.mask = 0; }
}
// true: image `bit` of this block has to be packed now (and counts as packed from here on)
bool fused_images_claim(const dsph_plan* plan, const void* ws, uint32_t bit) {
  FusedPlan* fp = plan->fused;
  if (!fp || !ws) return true;
  std::lock_guard<std::mutex> lock(fp->img_mu);
  auto it = fp->images.find(ws);
  if (it == fp->images.end()) return true;
  if (it->second.mask & bit) return false;
  it->second.mask |= bit;
  return true;
}
void fused_images_forget(const dsph_plan* plan, const void* ws) {
  FusedPlan* fp = plan->fused;
  if (!fp || !ws) return;
  std::lock_guard<std::mutex> lock(fp->img_mu);
  fp->images.erase(ws);
}
uint64_t fused_images_key(int32_t Fin, int32_t Fin_w, int32_t Fout, int32_t K, int32_t ld, int32_t precision, bool cheb, bool many, bool pack) {
  // (values beyond the fields' widths alias at worst to "another key": a re-pack)
  return ((uint64_t)(Fin & 0xfff)) | ((uint64_t)(Fin_w & 0xfff) << 12) | ((uint64_t)(Fout & 0xff) << 24) | ((uint64_t)(K & 0x3f) << 32) |
         ((uint64_t)(ld & 0xffff) << 38) | ((uint64_t)(precision & 3) << 54) | ((uint64_t)cheb << 56) | ((uint64_t)many << 57) |
         ((uint64_t)pack << 58) | (1ull << 63);
}

// The side stream and its two events exist only on plans that fork (a network holds dozens of plans, most of which
// never do): created by dsph_plan_prepare when the prepared tables call for it, or by the first forward that wants to fork --
// unless that forward is being captured into a graph, in which case it runs on the one stream.  Under fork_mu.
static bool side_stream_ready(const dsph_plan* plan, FusedPlan* fp, hipStream_t caller, bool may_create) {
  if (fp->side) return true;
  if (fp->side_failed || !may_create) return false;
  if (caller != nullptr) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(caller, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return false;
  }
  DeviceGuard guard(plan->device);
  hipStream_t st = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (!guard.ok || hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { fp->side_failed = true; return false; }
  if (hipEventCreateWithFlags(&e0, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&e1, hipEventDisableTiming) != hipSuccess) {
    if (e0) (void)hipEventDestroy(e0);
    (void)hipStreamDestroy(st);
    fp->side_failed = true;
    return false;
  }
  fp->ev_fork = e0;
  fp->ev_join = e1;
  fp->side = st;
  return true;
}

// LDS planes are sized at compile time: 576 rows (a 16x16 tile with a 4-ring halo), 768 or 1024
static int plane_rows_for(int rmax, int emax, int wt) {
  if (rmax <= 576 && emax <= 512) return 576;
  if (rmax <= 768 && emax <= 768) return 768;
  if (rmax <= 928 && emax <= 928) return 928;
  if (rmax <= 1024 && emax <= 1024) return 1024;
  return (rmax <= 1168 && emax <= 1024 && wt == 9) ? 1168 : 0;  // (K = 10 on the 8-neighbour grid: 34 x 34 rows, ELL rows on the inner 32 x 32; width 9 only)
}

// Layers the BFS-tile kernel runs with four maps per item (FusedArgs::pack): at most four input channels (padded to four),
// at most 16 output columns.  Its weight image then has two column blocks whatever the layer's width.
static int bfs_packs(int32_t Fin, int32_t Fout) { return Fin == 4 && Fout <= 16 ? 4 : (Fin == 8 && Fout <= 32 ? 2 : 0); }

// The packed weight images of one 64-column block of a layer, back to back in the workspace:
//   BFS-tile | structured-tile | strip pairs | input-side strips | K = 5 quad strips | K = 8 quad strips
// as byte offsets into the block (a `wimg` / `wfrag` pointer is the block's base + one of them) and the block's size.  Callers
// hold workspaces of dsph_workspace_bytes and, with DSPH_FWD_KEEP_WEIGHTS, packed images at these very offsets.
struct WeightImages {
  size_t bfs = 0, structured, strip, istrip, qstrip, qstrip8, total;
  size_t bfs_bytes;  // the BFS-tile kernel's image: what it also keeps in the LDS next to the planes
  WeightImages(int32_t Fin, int32_t Fout, int32_t K) {
    const int C = (Fin + FUSED_CH - 1) / FUSED_CH, NB = bfs_packs(Fin, Fout) ? 2 : (Fout + 31) / 32;
    bfs_bytes = (size_t)K * C * NB * 2048;
    structured = bfs + bfs_bytes;
    strip = structured + struct_wfrag_bytes(Fin, Fout, K);
    istrip = strip + strip_wimg_bytes(Fin, Fout, K);
    qstrip = istrip + 2 * istrip_wimg_bytes(K, DSPH_PREC_BF16X6);  // (the largest of the three arithmetics, two 32-column blocks)
    qstrip8 = qstrip + (qstrip_shape_ok(Fin, Fout, K) ? qstrip_wimg_bytes() : 0);
    total = qstrip8 + (qstrip8_shape_ok(Fin, Fout, K) ? qstrip8_wimg_bytes() : 0);
  }
};

// A layer's workspace: one block of images per 64 output columns (so that the packed images of ALL blocks survive the call:
// DSPH_FWD_KEEP_WEIGHTS), each block sized for the layer's widest one, and behind them the zero-padded copy of x when the
// layer's channel count is not a multiple of four.
struct LayerWorkspace {
  size_t block, padded_x, total;  // a block's stride; offset of the padded copy = end of the blocks; everything
  LayerWorkspace(const dsph_plan* plan, int64_t N, int32_t Fin, int32_t Fout, int32_t K) {
    const int32_t Fp = pad4(Fin);
    block = WeightImages(Fp, std::min(Fout, 64), K).total;
    padded_x = (size_t)((Fout + 63) / 64) * block;
    total = padded_x + (Fp != Fin ? (size_t)N * (size_t)plan->n_cols * (size_t)Fp * 4 : 0);
  }
};
size_t fused_workspace_bytes(const dsph_plan* plan, int64_t N, int32_t Fin, int32_t Fout, int32_t K, int32_t) {
  return LayerWorkspace(plan, N, Fin, Fout, K).total;
}

// The structured-tile kernel addresses x by 32-bit byte offsets inside a map: larger maps take BFS tables throughout.
static bool want_full(const dsph_plan* plan, int32_t Fin, bool full) {
  return full || (uint64_t)plan->n_cols * (uint64_t)Fin * 4ull >= (1ull << 32);
}
// tiles of the structured kernel, class R or T (what a fork and a deferred activation ask about; none in a full table)
static bool has_struct_tiles(const FusedTiles& ft) { return ft.r.n + ft.t.tiles.n > 0; }

// The tables a launch of this shape runs on (full: those of the planes and weight-gradient modes); nullptr: the fused kernels
// do not take the shape on this plan.  One look-up: whoever needs the tables after asking "supported" asks here.
static const FusedTiles* tiles_for(const dsph_plan* plan, int32_t Fin, int32_t Fout, int32_t K, bool full) {
  if (!plan->fused || plan->fused->wide) return nullptr;
  if (K < 2 || K - 1 > FUSED_DMAX) return nullptr;
  if (Fin % 4 != 0 || Fin < 4 || Fout < 1) return nullptr;  // Fout > 64: one launch per 64-column block
  const FusedTiles& ft = get_tiles(plan, K - 1, want_full(plan, Fin, full));
  if (!ft.ok) return nullptr;
  if (has_struct_tiles(ft) && !struct_shape_ok(Fin, std::min(Fout, 64), K)) return nullptr;
  if (ft.part.n == 0) return &ft;  // every tile is class R
  const int pr = plane_rows_for(ft.rmax, ft.emax, ft.width);
  if (pr == 0) return nullptr;
  // (the weight fragments need not fit beside the planes: the forward then reads them from global memory, cheb_fused_kernel's
  // WG variant; the planes and weight-gradient modes hold no weights)
  return (size_t)2 * pr * FUSED_CH * 4 + FUSED_BIAS_BYTES <= (size_t)LDS_BYTES ? &ft : nullptr;
}

int fused_dmax() { return FUSED_DMAX; }
int fused_num_cu(const dsph_plan* plan) { return plan->fused ? plan->fused->num_cu : 256; }

// Depth-1 breadth-first tables of a whole graph too wide for the fused kernels: what the tiled step gathers from (cheb_tstep.hip)
bool fused_tstep_tables(const dsph_plan* plan, TStepTables* out) {
  if (!plan->fused || !plan->fused->wide || plan->n_cols != plan->n_rows || !plan->levels.empty()) return false;
  const FusedTiles& ft = get_tiles(plan, 1, true);
  if (!ft.ok || ft.rmax > 768 || ft.part.n != ft.ntiles) return false;  // (TS_RMAX of cheb_tstep.hip)
  out->tile_off = ft.d_tile_off;
  out->ring_end = ft.d_ring_end;
  out->ell_off = ft.d_ell_off;
  out->region = ft.d_region;
  out->lcols = ft.d_lcols;
  out->lvals = ft.d_lvals;
  out->ntiles = ft.ntiles;
  out->width = ft.width;
  return true;
}

// (the forward takes any Fin >= 1: pad4)
bool fused_supported(const dsph_plan* plan, int32_t Fin, int32_t Fout, int32_t K) {
  return Fin >= 1 && tiles_for(plan, pad4(Fin), Fout, K, false) != nullptr;
}

// ... and with the BFS-tile kernel's weight fragments resident in the LDS (its fast variant: what "supported" meant before the
// WG variant existed; the K > 5 routing of dsphere_api.hip prefers the chain of passes to the WG variant)
bool fused_weights_resident(const dsph_plan* plan, int32_t Fin, int32_t Fout, int32_t K) {
  const FusedTiles* ft = Fin >= 1 ? tiles_for(plan, pad4(Fin), Fout, K, false) : nullptr;
  if (!ft) return false;
  if (ft->part.n == 0) return true;
  const int pr = plane_rows_for(ft->rmax, ft->emax, ft->width);
  return (size_t)2 * pr * FUSED_CH * 4 + WeightImages(pad4(Fin), std::min(Fout, 64), K).bfs_bytes + FUSED_BIAS_BYTES <= (size_t)LDS_BYTES;
}

int fused_prepare(const dsph_plan* plan, int32_t K, int32_t Fin, int32_t flags) {
  FusedPlan* fp = plan->fused;
  if (fp && fp->wide) {  // the tiled step's tables, so that the first forward does not build them
    TStepTables tb;
    if (K >= 2) (void)fused_tstep_tables(plan, &tb);
  } else {
    if (!fp || K < 2 || K - 1 > FUSED_DMAX) return DSPH_OK;  // nothing to build: the unfused path serves it
    const FusedTiles& ftp = get_tiles(plan, K - 1, want_full(plan, pad4(std::max(Fin, 1)), false));
    if (ftp.ok && plan->opt.fork && has_struct_tiles(ftp) && ftp.part.n > 0) {  // a forward of this K may fork: the side stream exists before it
      std::lock_guard<std::mutex> lock(fp->fork_mu);
      (void)side_stream_ready(plan, fp, nullptr, true);
    }
    // (the K = 5 quad strips' image of L~ in the Chebyshev basis, the default one: a captured first forward finds it)
    if (ftp.ok && qstrip_shape_ok(Fin, 64, K) && plan->opt.strip_form == 0) (void)qstrip_cimage(plan, ftp, true, nullptr);
    if (flags & DSPH_PREPARE_BACKWARD) {
      (void)get_tiles(plan, K - 1, true);
      (void)fused_symmetric(plan);  // (what the quad-strip weight gradient asks; the host arrays may be released below)
    }
  }
  if (flags & DSPH_PREPARE_RELEASE_HOST) {
    std::lock_guard<std::mutex> lock(fp->mu);
    std::vector<int32_t>().swap(fp->h_cols);
    std::vector<float>().swap(fp->h_vals);
    fp->host_released = true;
  }
  return DSPH_OK;
}

// ------------------------------------------------------------------------------------------
// routing: which kernel takes which tiles of a call
// ------------------------------------------------------------------------------------------

enum class Mode { forward, planes, wgrad };
enum class Strips { none, pairs, quad, input };  // strip pairs (cheb_strip), K = 5 quad strips (cheb_qstrip), input-side strips (cheb_istrip)

// What one fused launch is -- the forward of one 64-column block of a layer, or the planes / weight-gradient mode of the
// BFS-tile kernel -- and with that everything its routing depends on besides the plan's tables.  A launch fills all of it; a
// query of the plan fills in what it was asked, and the defaults are what it assumes for the rest: a whole-map forward in the
// Chebyshev basis with no activation and no pooling, y on a 16-byte boundary.
struct FusedRequest {
  Mode mode = Mode::forward;
  int64_t N = 1;
  int32_t Fin = 0;     // channels of x as the kernels see it (a multiple of four)
  int32_t Fin_w = 0;   // channels of w: fewer than Fin when x is a zero-padded copy
  int32_t Fout = 0;    // the columns of THIS launch (one 64-column block of the layer)
  int32_t ld = 0;      // the layer's row stride of y, w, dy and dw
  int32_t K = 0, precision = DSPH_PREC_BF16X3, act = DSPH_ACT_NONE, part = 0;
  float alpha_rest = 2.f, beta_rest = 1.f;
  const FusedPool* pool = nullptr;       // conv + pool: the kernels store the pooled map (launch_cheb_fused)
  const TileList* only_tiles = nullptr;  // weight-gradient mode next to the quad-strip gradient: the BFS-tile kernel on these tiles only
  const dsph_plan* plan = nullptr;
  const float* x = nullptr; const float* w = nullptr; const float* bias = nullptr; float* y = nullptr;
  unsigned char* ws = nullptr;  // this block's weight images (WeightImages)
  hipStream_t stream = nullptr;
};

struct Route {
  const FusedTiles& ft;      // the tables it was computed on: nothing below a route looks them up again
  bool has_struct, has_bfs;  // work for the structured half (forward only) / tiles of this part in the BFS-tile kernel's own list
  Strips strips;             // the strip kernel that takes the rectangles of this shape and batch ...
  bool run_strips;           // ... and whether this part launches it (rectangles are interior tiles: PART_BOUNDARY has none)
  const TileList* r;         // structured kernel without tables: class R, or what the strips leave of it
  const TileTables* t;       // structured kernel with tables: class T, or what the quad strips leave of it
  bool q8;                   // the K = 8 quad strips take their rectangles
  const int32_t* bfs_tiles;  // BFS-tile kernel: its tiles of this part (nullptr: every tile of the plan, no list) ...
  int bfs_n;                 // ... what the K = 8 strips leave of them, or the caller's only_tiles
  int pack;                  // maps per item of the BFS-tile kernel (FusedArgs::pack; 0: one)
  int pr;                    // its plane-row variant (plane_rows_for; 0: none)
};

// The strips are worth it for this batch: a strip step (48 output pixels of one row, one map) takes a workgroup
// ~3.0 us, a 256-pixel tile of one map takes the tile kernels ~18.7 us of a CU (both measured at the headline shape): in units
// of 0.1 us,   strips: (steps of the busiest workgroup, strip_makespan) x 30      tile kernels: tiles x N x 187 / CUs,
// with 3 % in favour of the tile kernels.  Small maps (fewer items than CUs) and ragged masks at small batches lose that
// comparison and keep their tiles on the tile kernels.  The rule depends on the batch and on the device's CU count, so the
// same map can be summed in two different orders at two batch sizes (both within the tolerance of the precision); a caller
// that needs batch- or shard-invariant bits fixes the choice per plan: dsph_plan_set_option(DSPH_OPT_STRIPS, 1 always | 2 never).
static bool use_qstrips(const dsph_plan* plan, const FusedTiles& ft, const FusedRequest& q) {
  return plan->opt.strip_form == 0 && ft.q5.n > 0 && qstrip_shape_ok(q.Fin, q.Fout, q.K);
}
static bool strips_apply(const dsph_plan* plan, const FusedTiles& ft, const FusedRequest& q, bool quad) {
  if (!((quad || ft.n_pairs > 0) && (q.precision == DSPH_PREC_BF16X3 || (q.precision == DSPH_PREC_F16X3 && quad)) &&
        strip_shape_ok(q.Fin, q.Fout, q.K) && q.ld % 4 == 0 && plan->n_cols * (int64_t)std::max(q.Fin, q.ld) * 4 < (1ll << 32)))
    return false;
  if (ft.strip_forced) return true;
  FusedPlan* fp = plan->fused;
  const int64_t N = q.N;
  if (quad) {
    // (a quad-strip step takes 2.8 us, a tile-map 18.7; the tape of rows is cut evenly, so the span is a formula)
    if (N < 1) return false;
    const int64_t span = qstrip_split(fp->num_cu, ft.q5.tape_rows, N, ft.q5.tape_rows / std::max(1, ft.q5.n), nullptr, nullptr, nullptr);
    return span * 28 * 103 < ft.q5.n_tiles * N * 187 / fp->num_cu * 100;
  }
  const std::vector<int32_t>& steps = ft.strip_steps;
  if (N < 1 || (int64_t)steps.size() * N > (1ll << 24)) return false;
  int64_t span;
  {
    std::lock_guard<std::mutex> lock(fp->mu);
    auto it = ft.strip_span.find(N);
    if (it == ft.strip_span.end()) it = ft.strip_span.emplace(N, strip_makespan(steps, N, fp->num_cu)).first;
    span = it->second;
  }
  return span * 30 * 103 < ft.n_strip_tiles * N * 187 / fp->num_cu * 100;
}

// The K = 8 quad strips take their rectangles for a whole-map forward of their shape (32 -> 32, three-term bf16, Chebyshev basis,
// bias / ReLU epilogue) when the strips pay for the batch by the same kind of rule (a step 2.6 us, a tile on the breadth-first
// kernel 27.5 us of a CU); DSPH_OPT_STRIPS 1 / 2: always / never.
static bool q8_applies(const dsph_plan* plan, const FusedTiles& ft, const FusedRequest& q) {
  // (no limit on the size of a map: this kernel forms its addresses in 64 bits -- configs[3] is 6.4 GB of x)
  // (ld == Fout: the layer IS 32 columns wide -- the last 32 columns of a wider layer would find no room for this kernel's weight
  // image in their block of the workspace, which is sized for 64-column blocks)
  if (ft.q8.n == 0 || !qstrip8_shape_ok(q.Fin, q.Fout, q.K) || (q.precision != DSPH_PREC_BF16X3 && q.precision != DSPH_PREC_F16X3) ||
      q.ld != q.Fout || q.N < 1)
    return false;
  if (plan->opt.strips == 1) return true;
  const int64_t span = qstrip8_split(plan->fused->num_cu, ft.q8.tape_rows, q.N, ft.q8.tape_rows / std::max(1, ft.q8.n), nullptr, nullptr, nullptr);
  return span * 26 * 103 < ft.q8.n_tiles * q.N * 275 / plan->fused->num_cu * 100;
}

// The input-side strip kernel takes the rectangles of every layer with at most 16 input channels (any arithmetic, K = 2 .. 5,
// any output width), unless DSPH_OPT_STRIPS says never.  No cost rule: its workers are single waves and the kernel cuts the
// strips into as many row segments as the batch needs, so small maps fill the device too (istrip_segments).
static bool istrips_apply(const dsph_plan* plan, const FusedTiles& ft, const FusedRequest& q) {
  return ft.n_ipairs > 0 && plan->opt.strips != 2 && istrip_shape_ok(q.Fin, q.K) && q.Fout % 4 == 0 && q.ld % 4 == 0;
}
static int istrip_nseg(const dsph_plan* plan, const FusedTiles& ft, int64_t N, int D, bool narrow) {
  FusedPlan* fp = plan->fused;
  std::lock_guard<std::mutex> lock(fp->mu);
  const int64_t key = 2 * N + (narrow ? 1 : 0);
  auto it = ft.iseg.find(key);
  if (it == ft.iseg.end()) it = ft.iseg.emplace(key, istrip_segments(ft.ipair_h, ft.ipair_second, N, fp->num_cu, D, narrow)).first;
  return it->second;
}

// THE rule: which kernel takes which tiles of this launch.  The launches below, dsph_plan_strip_tiles, fused_pool_ok and
// fused_qwgrad_applies all read its answer; none restates a condition of it.
// forked: this launch is one half of a forked forward.
static Route make_route(const dsph_plan* plan, const FusedTiles& ft, const FusedRequest& q, bool forked) {
  const bool fwd = q.mode == Mode::forward, y_aligned = (reinterpret_cast<uintptr_t>(q.y) & 15) == 0;
  // (both quad-strip kernels load their four bias values per lane as one 16-byte piece; every other kernel reads bias by the element)
  const bool bias_aligned = (reinterpret_cast<uintptr_t>(q.bias) & 15) == 0;
  const bool plain_epilogue = q.act == DSPH_ACT_NONE || q.act == DSPH_ACT_RELU;
  Route rt{ft};
  rt.has_struct = fwd && has_struct_tiles(ft);
  rt.has_bfs = ft.part.count(q.part) > 0;
  // rectangles of interior class-R tiles: a strip kernel, when it has this shape (the strip pairs and the quad strips read w
  // and x with the same channel count; all of them store y in 16-byte pieces); the class-R list shrinks to the rest
  const bool quad = use_qstrips(plan, ft, q);
  rt.strips = Strips::none;
  if (fwd && strips_apply(plan, ft, q, quad) && q.Fin_w == q.Fin && y_aligned && (!quad || bias_aligned)) rt.strips = quad ? Strips::quad : Strips::pairs;
  else if (fwd && istrips_apply(plan, ft, q) && y_aligned) rt.strips = Strips::input;
  rt.run_strips = rt.strips != Strips::none && q.part != 2;
  // (the quad strips took class-T tiles too: their own rest lists)
  rt.r = rt.strips == Strips::quad ? &ft.qrrest : (rt.strips != Strips::none ? &ft.rrest : &ft.r);
  rt.t = rt.strips == Strips::quad ? &ft.qt : &ft.t;
  // K = 8, 32 -> 32: the rectangles of depth-7 regular tiles on the quad strips, the rest of the tiles on the BFS-tile kernel
  rt.q8 = fwd && q.part != 2 && !q.pool && !forked && q.Fin_w == q.Fin && q.beta_rest != 0.f && plain_epilogue && y_aligned && bias_aligned && q8_applies(plan, ft, q);
  // part: 0 all tiles, 1 interior tiles (no row of another rank in their region), 2 boundary tiles
  // the BFS-tile kernel handles the tiles of ft.part (every tile of a full table, the class-G ones otherwise)
  rt.bfs_tiles = q.part == 0 && ft.part.n == ft.ntiles ? nullptr : ft.part.ptr(q.part);
  rt.bfs_n = ft.part.count(q.part);
  if (rt.q8) {  // (part 0: every tile the strips leave; part 1: the interior ones of them -- the boundary tiles are never the strips')
    rt.bfs_tiles = ft.q8rest.ptr(q.part);
    rt.bfs_n = ft.q8rest.count(q.part);
  }
  if (q.only_tiles) {  // (the strips' pixels go to cheb_qwgrad.hip: launch_cheb_fused_qwgrad)
    rt.bfs_tiles = q.only_tiles->d;
    rt.bfs_n = q.only_tiles->n;
  }
  // four maps per item where the layer has at most four input channels and 16 output columns (a single map gains nothing from two column blocks)
  rt.pack = (plan->opt.pack && fwd && q.N >= 2) ? bfs_packs(q.Fin, q.Fout) : 0;
  rt.pr = plane_rows_for(ft.rmax, ft.emax, ft.width);
  return rt;
}

// conv + HealpyPool(p = 1) in one forward (launch_cheb_fused with a FusedPool): the input-side strip kernels, the structured
// kernel and the BFS-tile kernel store the pooled map themselves.  Every layer whose tiles those kernels take -- not the
// 64 -> 64 shape on maps large enough for the Clenshaw strips --, whole unsharded maps of whole tiles,
// a width that is a multiple of four, bias and ReLU only (the other activations run as a separate pass over the full-resolution map).
bool fused_pool_ok(const dsph_plan* plan, int64_t N, int32_t Fin, int32_t Fout, int32_t K, int32_t act) {
  if (!plan->fused || N < 1 || !(act == DSPH_ACT_NONE || act == DSPH_ACT_RELU)) return false;
  if (!plan->levels.empty() || plan->n_cols != plan->n_rows || plan->n_rows % FUSED_P != 0 || K < 2 || K - 1 > FUSED_DMAX) return false;
  const FusedTiles* ft = Fin >= 1 ? tiles_for(plan, pad4(Fin), Fout, K, false) : nullptr;
  if (!ft || Fout % 4 != 0) return false;  // (pooled stores are 16 bytes wide)
  // the Clenshaw strip kernel has no pooled epilogue: not where it would take tiles.  Asked for the three-term bf16 arithmetic
  // (either precision could be asked for), the layer's first block, an aligned y and an x that needs no padding.
  FusedRequest q;
  q.N = N; q.Fin = q.Fin_w = pad4(Fin); q.Fout = std::min(Fout, 64); q.ld = Fout; q.K = K; q.precision = DSPH_PREC_BF16X3;
  const Strips s = make_route(plan, *ft, q, false).strips;
  return s != Strips::pairs && s != Strips::quad;
}

// tiles a forward of this shape hands to a strip kernel: the route of the layer's first 64-column block (a layer with
// Fout = 96 runs its first block through the strips and reports them; one with Fout < 64 has none on the Clenshaw strips).
// Assumed, because the question does not say: a whole-map forward in the Chebyshev basis with no activation, an aligned y.
int64_t fused_strip_tiles(const dsph_plan* plan, int64_t N, int32_t Fin, int32_t Fout, int32_t K, int32_t precision) {
  if (!plan->fused || K < 2 || K - 1 > FUSED_DMAX) return 0;
  const FusedTiles& ft = get_tiles(plan, K - 1, want_full(plan, pad4(Fin), false));
  if (!ft.ok) return 0;
  FusedRequest q;
  q.N = N; q.Fin = pad4(Fin); q.Fin_w = Fin; q.Fout = std::min(Fout, 64); q.ld = Fout; q.K = K; q.precision = precision;
  const Route rt = make_route(plan, ft, q, false);
  if (rt.q8) return ft.q8.n_tiles;
  return rt.strips == Strips::quad ? ft.q5.n_tiles : (rt.strips != Strips::none ? ft.n_strip_tiles : 0);
}

// ------------------------------------------------------------------------------------------
// the small kernels of this file: zero-padded copy of x, weight preparation, reduction of the weight gradient's slabs
// ------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void fused_pad_kernel(const float* __restrict__ x, float4* __restrict__ out, int64_t rows,
                                                        int Fin, int Q) {  // out[r][q] <- x[r][4q .. 4q+3], zeros past Fin
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < rows * Q; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / Q;
    const int c = 4 * (int)(i - r * Q);
    const float* __restrict__ src = x + r * Fin + c;
    float4 v;
    v.x = src[0];
    v.y = c + 1 < Fin ? src[1] : 0.f;
    v.z = c + 2 < Fin ? src[2] : 0.f;
    v.w = c + 3 < Fin ? src[3] : 0.f;
    out[i] = v;
  }
}

// Weight fragments in MFMA operand order (dsphere_wfrag.h: the 32x32 geometry), one 2 KiB block per (order k, slice c, column
// block nb): WF_BF16X3 or WF_FP32_STEPS of w[(16 c + inner)*K + k][32 nb + col].
// pack (four maps per item, FusedArgs::pack): one slice, two column blocks, block diagonal (wf_gather_pack).
__global__ __launch_bounds__(256) void fused_wprep_kernel(const float* __restrict__ w,
                                                          unsigned char* __restrict__ out, int Fin,
                                                          int Fout, int K, int C, int NB, int prec, int ld, int pack) {
  const int blk = blockIdx.x;  // (k*C + c)*NB + nb
  const int nb = blk % NB, c = (blk / NB) % C, k = blk / (NB * C);
  for (int e = threadIdx.x; e < WF_ELEMS; e += 256) {
    const WfElem p = wf_elem32(e);
    wf_put(out + (size_t)blk * 2 * WF_FRAG, prec == DSPH_PREC_BF16X3 ? WF_BF16X3 : WF_FP32_STEPS, p.l, p.j,
           wf_gather_pack(w, c * FUSED_CH + p.inner, 32 * nb + p.col, Fin, Fout, K, k, ld, pack));
  }
}

// dw[(f*K + k)*Fout + o] = sum over slabs, in a fixed order (deterministic): sixteen lanes per element, lane p sums the slabs
// p, p + 16, ... in ascending order, the sixteen partial sums are added pairwise in a fixed tree.  (One thread per element with
// a serial loop over 512 slabs took 0.14 ms at 16 -> 32: more than a seventh of that layer's weight gradient.)
// mirror_grid > 0 (the bf16 arithmetic): the slabs of the odd workgroups blockIdx.x of a grid of that many hold -dW
// (cheb_fused_kernel.h, weight-gradient mode) and are subtracted.
__global__ __launch_bounds__(256) void fused_wgrad_reduce_kernel(const float* __restrict__ slabs, float* __restrict__ dw,
                                                                 int nslabs, int Fin, int Fout, int K, int C, int ld, int mirror_grid) {
  __shared__ float part[16][17];
  const int el = threadIdx.x & 15, p = threadIdx.x >> 4;
  const int e = blockIdx.x * 16 + el;
  const bool live = e < Fin * K * Fout;
  const int o = live ? e % Fout : 0, fk = live ? e / Fout : 0, k = fk % K, f = fk / K;
  const size_t slab = (size_t)C * K * 16 * 64;
  const size_t off = ((size_t)((f >> 4) * K + k) * 16 + (f & 15)) * 64 + o;
  float s = 0.f;
  if (live)
    for (int i = p; i < nslabs; i += 16) {
      const float v = slabs[(size_t)i * slab + off];
      s += (mirror_grid > 0 && (((i >> 1) % mirror_grid) & 1)) ? -v : v;
    }
  part[p][el] = s;
  __syncthreads();
  if (p == 0 && live) {
    float v[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = part[q][el];
#pragma unroll
    for (int h = 8; h >= 1; h >>= 1)
#pragma unroll
      for (int q = 0; q < h; ++q) v[q] += v[q + h];
    dw[(size_t)fk * ld + o] = v[0];
  }
}

int launch_fused_pad(const float* x, float* xp, int64_t rows, int32_t Fin, int32_t Fp, hipStream_t stream) {
  const int64_t work = rows * (Fp / 4);
  hipLaunchKernelGGL(fused_pad_kernel, dim3((unsigned)std::min<int64_t>((work + 255) / 256, 65536)), dim3(256), 0, stream, x,
                     reinterpret_cast<float4*>(xp), rows, (int)Fin, (int)(Fp / 4));
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

// ------------------------------------------------------------------------------------------
// launches
// ------------------------------------------------------------------------------------------

// Arithmetic of the structured-tile, strip-pair and input-side strip kernels for a request: DSPH_PREC_F16X3 is the quad strips'
// own; every other kernel of the forward runs the six-term split then (same accuracy)
static int32_t struct_arithmetic(int32_t precision) { return precision == DSPH_PREC_F16X3 ? DSPH_PREC_BF16X6 : precision; }
// ... and of the BFS-tile kernel, which has two contraction arithmetics: the six-term split of the structured kernel is fp32-equivalent
static int32_t bfs_arithmetic(int32_t precision) {
  return struct_arithmetic(precision) == DSPH_PREC_BF16X6 ? DSPH_PREC_FP32 : precision;
}

// The refusal of a pointer that the fused kernels would load or store in 16-byte pieces: it names the pointer and the requirement.
static bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
static int refuse_misaligned(const char* who) {
  set_error("cheb_fused: %s must be 16-byte aligned (the fused kernels access it in 16-byte pieces; DSPH_ALGO_UNFUSED takes any 4-byte-aligned pointer)", who);
  return DSPH_E_BADARG;
}

// What every launch checks first: the shape runs on these tables (ft: tiles_for), the block's images fit, the pointers the
// kernels load and store in 16-byte pieces are aligned (out: the planes, or the slabs of the weight gradient).
static int check_request(const FusedRequest& rq, const FusedTiles* ft, size_t ws_bytes, size_t ws_need, const void* out) {
  if (!ft) {
    set_error("cheb_fused: plan/shape not supported");
    return DSPH_E_UNSUPPORTED;
  }
  if (ws_need > 0 && (!rq.ws || ws_bytes < ws_need)) {
    set_error("cheb_fused: workspace %zu < %zu", ws_bytes, ws_need);
    return DSPH_E_WORKSPACE;
  }
  const char* who = misaligned(rq.x) ? "x" : misaligned(rq.ws) ? "the workspace" : misaligned(out) ? (rq.mode == Mode::planes ? "planes" : "the workspace") : nullptr;
  if (who) return refuse_misaligned(who);
  return DSPH_OK;
}

// the part of a strip or tile launch that is the same for every kernel of the call
static LaunchBase launch_base(const FusedRequest& rq) {
  LaunchBase b;
  b.x = rq.x; b.w = rq.w; b.bias = rq.bias; b.y = rq.y;
  b.gvals8 = rq.plan->fused->d_gvals8;
  b.gdiag = rq.plan->fused->d_gdiag;
  b.x_rows = rq.plan->n_cols; b.y_rows = out_rows(rq.plan); b.N = rq.N;
  b.act = rq.act; b.ld = rq.ld; b.num_cu = rq.plan->fused->num_cu;
  b.cheb = rq.beta_rest != 0.f;
  if (rq.pool != nullptr) {
    b.pool = rq.pool->type;
    b.ypool = rq.pool->y;
    b.ypool_rows = rq.plan->n_rows / 4;
  }
  return b;
}

// the strip kernel of the route on the rectangles
static int launch_strips(const FusedRequest& rq, const Route& rt, const WeightImages& img, const LaunchBase& base) {
  const dsph_plan* plan = rq.plan;
  const FusedTiles& ft = rt.ft;
  if (rt.strips == Strips::quad) {
    QStripLaunch qs;
    static_cast<LaunchBase&>(qs) = base;
    qs.wimg = rq.ws + img.qstrip;
    qs.strips = ft.q5.d_strips;
    qs.tab = ft.q5.d_tab;
    qs.prefix = ft.q5.d_prefix;
    qs.tape_rows = ft.q5.tape_rows;
    qs.nstrips = ft.q5.n; qs.Fin = rq.Fin; qs.Fout = rq.Fout;
    qs.f16 = rq.precision == DSPH_PREC_F16X3;
    qs.f16_xexp = plan->opt.f16_xexp;
    qs.cimg = qstrip_cimage(plan, ft, base.cheb, rq.stream);
    if (!qs.cimg && plan->opt.qstrip_image == 1 && ft.q5.cimg_failed) {
      set_error("cheb_fused: DSPH_OPT_QSTRIP_IMAGE = on, and no memory for the image (%lld bytes)", (long long)ft.q5.cimg_rows * QS_CROWB);
      return DSPH_E_HIP;
    }
    qs.prep_weights = fused_images_claim(plan, rq.ws, IMG_QSTRIP);
    return launch_cheb_qstrip(qs, rq.stream);
  }
  if (rt.strips == Strips::pairs) {
    StripLaunch st;
    static_cast<LaunchBase&>(st) = base;
    st.wimg = rq.ws + img.strip;
    st.pairs = ft.d_pairs;
    st.npairs = ft.n_pairs; st.Fin = rq.Fin; st.Fout = rq.Fout; st.K = rq.K; st.precision = struct_arithmetic(rq.precision);
    st.prep_weights = fused_images_claim(plan, rq.ws, IMG_STRIP);
    return launch_cheb_strip(st, rq.stream);
  }
  IStripLaunch is;
  static_cast<LaunchBase&>(is) = base;
  is.wimg = rq.ws + img.istrip;
  is.pairs = ft.d_ipairs;
  is.npairs = ft.n_ipairs; is.Fin = rq.Fin; is.Fin_w = rq.Fin_w; is.Fout = rq.Fout; is.K = rq.K; is.precision = struct_arithmetic(rq.precision);
  // (row segments for the items the kernel will deal: maps, or pairs of maps in the one-channel kernel's pair mode)
  is.nseg = istrip_nseg(plan, ft, istrip_pairs(rq.Fin_w, rq.Fout) ? (rq.N + 1) / 2 : rq.N, rq.K - 1, istrip_narrow(rq.Fin_w));
  is.prep_weights = fused_images_claim(plan, rq.ws, IMG_ISTRIP);
  return launch_cheb_istrip(is, rq.stream);
}

// The structured half of a forward: the strip kernel on the rectangles, then the structured-tile kernel on the class-R tiles
// (without tables) and the class-T tiles (with per-tile tables) of the route.
static int forward_structured(const FusedRequest& rq, const Route& rt, const WeightImages& img) {
  const dsph_plan* plan = rq.plan;
  const LaunchBase base = launch_base(rq);
  if (rt.run_strips) {
    const int rc = launch_strips(rq, rt, img, base);
    if (rc != DSPH_OK) return rc;
  }
  StructLaunch sl;
  static_cast<LaunchBase&>(sl) = base;
  sl.wfrag = rq.ws + img.structured;
  sl.Fin = rq.Fin; sl.Fin_w = rq.Fin_w; sl.Fout = rq.Fout; sl.K = rq.K; sl.precision = struct_arithmetic(rq.precision);
  sl.allow_pack = plan->opt.pack;
  bool struct_prep = true;  // the first structured launch of this call packs the fragments, if the block lacks them
  if (rt.r->count(rq.part) > 0) {
    sl.tiles = rt.r->ptr(rq.part);
    sl.ntiles = rt.r->count(rq.part);
    sl.prep_weights = fused_images_claim(plan, rq.ws, IMG_STRUCT);
    struct_prep = false;
    const int rc = launch_cheb_struct(sl, rq.stream);
    if (rc != DSPH_OK) return rc;
  }
  if (rt.t->tiles.count(rq.part) > 0) {
    sl.tiles = rt.t->tiles.ptr(rq.part);
    sl.tabrow = rt.t->rows(rq.part);
    sl.tabvals = rt.t->vals(rq.part);
    sl.ntiles = rt.t->tiles.count(rq.part);
    sl.prep_weights = struct_prep && fused_images_claim(plan, rq.ws, IMG_STRUCT);
    const int rc = launch_cheb_struct(sl, rq.stream);
    if (rc != DSPH_OK) return rc;
  }
  return DSPH_OK;
}

static int fused_grid(const dsph_plan* plan, int ntiles) { return std::max(8, std::min(plan->fused->num_cu, (ntiles + 7) / 8 * 8)); }

// The BFS-tile kernel's arguments as far as every mode shares them: the request, the tables and the route's tile list.
// The mode adds its own: y / bias / act / weights (forward), planes_out, or dy and the slabs.
static FusedArgs fused_args(const FusedRequest& rq, const Route& rt) {
  const dsph_plan* plan = rq.plan;
  const FusedTiles& ft = rt.ft;
  const int C = (rq.Fin + FUSED_CH - 1) / FUSED_CH;
  FusedArgs args{};  // (planes_out, dy, slabs, wfrag_bytes: none until the mode sets its own)
  args.c_count = C;
  args.prow_stride = plan->n_cols;
  args.plane_stride = rq.N * plan->n_cols * (int64_t)rq.Fin;
  args.x = rq.x;
  args.bias = rq.bias;
  args.y = rq.y;
  args.wfrag = rq.ws;
  args.tile_off = ft.d_tile_off;
  args.ring_end = ft.d_ring_end;
  args.ell_off = ft.d_ell_off;
  args.region = ft.d_region;
  args.lcols = ft.d_lcols;
  args.lvals = ft.d_lvals;
  args.x_rows = plan->n_cols;
  args.y_rows = out_rows(plan);
  args.N = rt.pack ? (int)((rq.N + rt.pack - 1) / rt.pack) : (int)rq.N;  // (packed: groups of P maps)
  args.n_maps = (int)rq.N;
  args.pack = rt.pack;
  args.num_cu = plan->fused->num_cu;
  args.pool = rq.pool ? rq.pool->type : 0;
  args.ypool = rq.pool ? rq.pool->y : nullptr;
  args.ypool_rows = plan->n_rows / 4;
  args.Fin = rq.Fin;
  args.Fout = rq.Fout;
  args.ld = rq.ld;
  args.K = rq.K;
  args.tile_list = rt.bfs_tiles;
  args.ntiles = rt.bfs_n;
  args.nchunks = C;
  args.act = rq.act;
  args.alpha_rest = rq.alpha_rest;
  args.beta_rest = rq.beta_rest;
  return args;
}

// the instantiation of the BFS-tile kernel for plane rows pr and ELL width wt (cheb_fused_inst.hip)
static int launch_fused_variant(int pr, int wt, const FusedArgs& a, int nb, int prec, int grid, size_t lds, hipStream_t stream) {
#define DSPH_FUSED_CASE(PR, WT) \
  if (pr == PR && wt == WT) return launch_fused_##PR##_##WT(a, nb, prec, grid, lds, stream);
  DSPH_FUSED_CASE(576, 9)
  DSPH_FUSED_CASE(768, 9)
  DSPH_FUSED_CASE(928, 9)
  DSPH_FUSED_CASE(1024, 9)
  DSPH_FUSED_CASE(1168, 9)
  DSPH_FUSED_CASE(576, 12)
  DSPH_FUSED_CASE(768, 12)
  DSPH_FUSED_CASE(928, 12)
  DSPH_FUSED_CASE(1024, 12)
#undef DSPH_FUSED_CASE
  set_error("cheb_fused: no kernel for plane rows %d, width %d", pr, wt);
  return DSPH_E_UNSUPPORTED;
}

// the BFS-tile kernel on the route's tile list, in the forward (wfrag_bytes of weights in the LDS) or the planes mode
static int launch_bfs_tiles(const FusedRequest& rq, const Route& rt, FusedArgs& args, int nb, size_t wfrag_bytes) {
  if (args.ntiles == 0) return DSPH_OK;
  args.wfrag_bytes = (int)wfrag_bytes;
  const size_t lds = (size_t)2 * rt.pr * FUSED_CH * 4 + wfrag_bytes;
  return launch_fused_variant(rt.pr, rt.ft.width, args, nb, bfs_arithmetic(rq.precision), fused_grid(rq.plan, args.ntiles), lds, rq.stream);
}

// The BFS half of a forward: the class-G tiles on the BFS-tile kernel; at K = 8, 32 -> 32 the rectangles first, on the quad strips.
static int forward_bfs(const FusedRequest& rq, const Route& rt, const WeightImages& img) {
  const dsph_plan* plan = rq.plan;
  const int C = (rq.Fin + FUSED_CH - 1) / FUSED_CH;
  const int NB = rt.pack ? 2 : (rq.Fout + 31) / 32;  // (packed: two column blocks whatever the layer's width)
  if (fused_images_claim(plan, rq.ws, IMG_BFS)) {
    hipLaunchKernelGGL(fused_wprep_kernel, dim3(rq.K * C * NB), dim3(256), 0, rq.stream, rq.w, rq.ws + img.bfs, (int)rq.Fin_w, (int)rq.Fout,
                       (int)rq.K, C, NB, (int)bfs_arithmetic(rq.precision), (int)rq.ld, rt.pack);
    DSPH_HIP(hipGetLastError());
  }
  if (rt.q8) {
    QStrip8Launch q;
    static_cast<LaunchBase&>(q) = launch_base(rq);
    q.wimg = rq.ws + img.qstrip8;
    q.strips = rt.ft.q8.d_strips; q.tab = rt.ft.q8.d_tab; q.prefix = rt.ft.q8.d_prefix; q.tape_rows = rt.ft.q8.tape_rows;
    q.nstrips = rt.ft.q8.n; q.ld_w = rq.ld;
    q.f16 = rq.precision == DSPH_PREC_F16X3;
    q.f16_xexp = plan->opt.f16_xexp;
    q.prep_weights = fused_images_claim(plan, rq.ws, IMG_Q8);
    const int rc = launch_cheb_qstrip8(q, rq.stream);
    if (rc != DSPH_OK) return rc;
  }
  FusedArgs args = fused_args(rq, rt);
  return launch_bfs_tiles(rq, rt, args, NB, img.bfs_bytes);
}

// Forward of one 64-column block on the caller's stream: the structured half, then the BFS half.
static int forward_block(const FusedRequest& rq, const FusedTiles* ft, size_t ws_bytes) {
  const WeightImages img(rq.Fin, rq.Fout, rq.K);
  const int rc = check_request(rq, ft, ws_bytes, img.total, nullptr);
  if (rc != DSPH_OK) return rc;
  const Route rt = make_route(rq.plan, *ft, rq, false);
  if (rt.has_struct) {
    const int rc_s = forward_structured(rq, rt, img);
    if (rc_s != DSPH_OK) return rc_s;
    if (!rt.has_bfs) return DSPH_OK;
  }
  return forward_bfs(rq, rt, img);
}

// Whether the BFS half of a forward goes to the plan's side stream: worth its two event operations only when the structured
// launches run for a while, two tile-maps per CU and more -- BASELINE configs[0], 168 tile-maps, is 13 us faster without it,
// configs[1] 29 us faster with it.  Under a stream capture the fork and the join are edges of the graph and cost nothing at
// replay: every forward with both kinds of tiles forks there, provided the side stream exists already -- dsph_plan_prepare made it.
static bool fork_pays(const dsph_plan* plan, const FusedTiles& ft, int64_t N, int32_t part, hipStream_t stream) {
  FusedPlan* fp = plan->fused;
  if (!plan->opt.fork || !has_struct_tiles(ft) || ft.part.count(part) == 0) return false;
  if (N * (int64_t)(ft.r.n + ft.t.tiles.n) >= 2 * (int64_t)fp->num_cu) return true;
  if (!fp->side || stream == nullptr) return false;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(stream, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive;
}

// One block of a forked forward (the halves write disjoint tiles): the BFS half on the side stream, forked behind whatever the
// caller's stream holds so far and joined before this returns; the structured half on the caller's stream.  One route serves
// both.  *ran = false: no side stream, nothing was launched.
static int forward_block_forked(const FusedRequest& rq, const FusedTiles* ft, size_t ws_bytes, bool* ran) {
  FusedPlan* fp = rq.plan->fused;
  hipStream_t stream = rq.stream;
  std::unique_lock<std::mutex> lock(fp->fork_mu);
  *ran = side_stream_ready(rq.plan, fp, stream, true);
  if (!*ran) return DSPH_OK;
  DSPH_HIP(hipEventRecord(fp->ev_fork, stream));             // (nothing is on the side stream yet: a failure here or in the
  DSPH_HIP(hipStreamWaitEvent(fp->side, fp->ev_fork, 0));    //  next line leaves nothing to join)
  const WeightImages img(rq.Fin, rq.Fout, rq.K);
  int rc_b = check_request(rq, ft, ws_bytes, img.total, nullptr), rc_s = rc_b;
  hipError_t e_rec;
  if (rc_b == DSPH_OK) {
    const Route rt = make_route(rq.plan, *ft, rq, true);
    FusedRequest side = rq;
    side.stream = fp->side;
    rc_b = forward_bfs(side, rt, img);
    e_rec = hipEventRecord(fp->ev_join, fp->side);
    rc_s = forward_structured(rq, rt, img);
  } else {
    e_rec = hipEventRecord(fp->ev_join, fp->side);
  }
  // the join happens whatever went wrong in between: the side stream never outlives the call.  (Without the join
  // event the only way to join is to wait for the side stream on the host -- not while the caller is capturing, where
  // a synchronisation would invalidate the capture: the error goes back instead, the capture is lost either way.)
  hipError_t e_join = hipSuccess;
  if (e_rec == hipSuccess) e_join = hipStreamWaitEvent(stream, fp->ev_join, 0);
  else {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone) e_join = hipStreamSynchronize(fp->side);
  }
  if (rc_b != DSPH_OK || rc_s != DSPH_OK) fused_images_forget(rq.plan, rq.ws);
  if (rc_b != DSPH_OK) return rc_b;
  if (rc_s != DSPH_OK) return rc_s;
  if (e_rec != hipSuccess) return hip_fail(e_rec, "hipEventRecord(join)");
  if (e_join != hipSuccess) return hip_fail(e_join, "join of the side stream");
  return DSPH_OK;
}

int launch_cheb_fused(const dsph_plan* plan, const float* x, const float* w, const float* bias,
                      float* y, int64_t N, int32_t Fin, int32_t Fout, int32_t K, int32_t act,
                      int32_t precision, float alpha_rest, float beta_rest, void* workspace,
                      size_t workspace_bytes, hipStream_t stream, int32_t part, bool keep_weights, const FusedPool* pool) {
  if (pool != nullptr && !(part == 0 && fused_pool_ok(plan, N, Fin, Fout, K, act) && pool->y != nullptr && (pool->type == 1 || pool->type == 2))) {
    set_error("cheb_fused: this plan / shape has no fused pooling (whole unsharded maps, no or ReLU activation, not the Clenshaw strips' shape)");
    return DSPH_E_UNSUPPORTED;
  }
  // (the pooled stores are 16 bytes wide in every kernel, and the route is that of an aligned y)
  if (pool != nullptr && misaligned(pool->y)) return refuse_misaligned("y_pooled");
  if (pool != nullptr && misaligned(y)) return refuse_misaligned("y_scratch");
  const LayerWorkspace lw(plan, N, Fin, Fout, K);
  if (!workspace || workspace_bytes < lw.total) {
    set_error("cheb_fused: workspace %zu < %zu", workspace_bytes, lw.total);
    return DSPH_E_WORKSPACE;
  }
  // before the first launch (the padded copy of x below is stored in 16-byte pieces; an x with Fin % 4 != 0 is read by the element)
  if (misaligned(workspace)) return refuse_misaligned("the workspace");
  if (Fin == pad4(Fin) && misaligned(x)) return refuse_misaligned("x");
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  // Fin not a multiple of four: a zero-padded copy of x behind the weight images in the workspace (with a two-part
  // launch both parts copy: the halo rows arrive between them)
  const int32_t Fin_w = Fin;
  if (Fin != pad4(Fin)) {
    float* xp = reinterpret_cast<float*>(ws + lw.padded_x);
    const int rc = launch_fused_pad(x, xp, N * plan->n_cols, Fin, pad4(Fin), stream);
    if (rc != DSPH_OK) return rc;
    x = xp;
    Fin = pad4(Fin);
  }
  // the tables of the call, looked up once (nullptr: not a shape of the fused kernels -- the first block says so)
  const FusedTiles* ft = tiles_for(plan, Fin, Fout, K, false);
  // The structured-tile kernel fuses bias and ReLU; with any other activation both fused kernels write the pre-activation
  // and one elementwise pass finishes y (only when class-R tiles exist: the BFS-tile kernel knows every activation).
  // (two-part launches: each part writes the pre-activation of its tiles and then finishes exactly those tiles' rows)
  const bool defer_act = act != DSPH_ACT_NONE && act != DSPH_ACT_RELU && ft && has_struct_tiles(*ft);
  // structured launches and the BFS-tile launch write disjoint tiles: when a forward has both, the latter goes to the plan's
  // side stream (FusedPlan::side)
  const bool fork = ft && fork_pays(plan, *ft, N, part, stream);
  // more than 64 output columns: one launch per 64-column block (the recurrence is repeated; still one pass
  // over x per block instead of the unfused path's K planes through HBM)
  FusedRequest rq;
  rq.plan = plan; rq.x = x; rq.stream = stream;
  rq.N = N; rq.Fin = Fin; rq.Fin_w = Fin_w; rq.ld = Fout; rq.K = K; rq.precision = precision; rq.part = part;
  rq.act = defer_act ? DSPH_ACT_NONE : act;
  rq.alpha_rest = alpha_rest; rq.beta_rest = beta_rest;
  for (int32_t cb = 0; cb < Fout; cb += 64) {
    const FusedPool pool_blk{pool ? pool->y + cb : nullptr, pool ? pool->type : 0};  // (this block's columns of the pooled map)
    rq.w = w + cb; rq.bias = bias ? bias + cb : nullptr; rq.y = y + cb;
    rq.Fout = std::min<int32_t>(64, Fout - cb);
    rq.ws = ws + (size_t)(cb / 64) * lw.block;
    rq.pool = pool ? &pool_blk : nullptr;
    fused_images_begin(plan, rq.ws, fused_images_key(Fin, Fin_w, rq.Fout, K, Fout, precision, beta_rest != 0.f, N >= 2, plan->opt.pack),
                       keep_weights);
    bool forked = false;
    int rc = fork ? forward_block_forked(rq, ft, lw.block, &forked) : DSPH_OK;
    if (!forked) {
      rc = forward_block(rq, ft, lw.block);
      if (rc != DSPH_OK) fused_images_forget(plan, rq.ws);
    }
    if (rc != DSPH_OK) return rc;
  }
  if (pool != nullptr) {
    return DSPH_OK;  // (every kernel has stored its tiles pooled; y, the scratch of the C ABI, stays untouched)
  }
  if (defer_act) {
    if (part == 0) return launch_struct_act(y, N * out_rows(plan), Fout, Fout, act, stream);
    // a part finishes the rows of its own tiles only: INTERIOR and BOUNDARY can be issued in any order, repeated, or alone
    return launch_struct_act_tiles(y, ft->all.ptr(part), ft->all.count(part), N, out_rows(plan), Fout, Fout, act, stream);
  }
  return DSPH_OK;
}

// Planes mode of the same kernel: T_1 .. T_{K-1} of x, each (N, n_cols, Fin), valid on the plan's output rows.
bool fused_planes_supported(const dsph_plan* plan, int32_t Fin, int32_t K) { return tiles_for(plan, Fin, 1, K, true) != nullptr; }

int launch_cheb_fused_planes(const dsph_plan* plan, const float* x, float* planes_out, int64_t N, int32_t Fin,
                             int32_t K, float alpha_rest, float beta_rest, hipStream_t stream) {
  FusedRequest rq;
  rq.mode = Mode::planes;
  rq.plan = plan; rq.x = x; rq.stream = stream;
  rq.N = N; rq.Fin = rq.Fin_w = Fin; rq.Fout = rq.ld = 1; rq.K = K; rq.precision = DSPH_PREC_FP32;
  rq.alpha_rest = alpha_rest; rq.beta_rest = beta_rest;
  const FusedTiles* ft = tiles_for(plan, Fin, 1, K, true);
  const int rc = check_request(rq, ft, 0, 0, planes_out);
  if (rc != DSPH_OK) return rc;
  const Route rt = make_route(plan, *ft, rq, false);
  FusedArgs args = fused_args(rq, rt);
  args.planes_out = planes_out;
  return launch_bfs_tiles(rq, rt, args, 1, 0);
}

// ---- weight-gradient mode ------------------------------------------------------------------------------

// slices per launch: as many accumulator tiles (one per slice and order, 8 KiB each) as fit the LDS next to the planes
static int wgrad_slices_per_launch(const FusedTiles& ft, int32_t K) {
  const int pr = plane_rows_for(ft.rmax, ft.emax, ft.width);
  if (pr == 0) return 0;
  const long freeb = (long)LDS_BYTES - 2L * pr * FUSED_CH * 4;
  return (int)(freeb / ((long)K * WG_TILE_BYTES));
}

// the full tables a weight gradient of this shape runs on; nullptr: not on the fused kernel
static const FusedTiles* wgrad_tiles_for(const dsph_plan* plan, int32_t Fin, int32_t Fout, int32_t K) {
  const FusedTiles* ft = tiles_for(plan, Fin, Fout, K, true);
  return ft && wgrad_slices_per_launch(*ft, K) >= 1 ? ft : nullptr;
}
bool fused_wgrad_supported(const dsph_plan* plan, int32_t Fin, int32_t Fout, int32_t K) {
  return wgrad_tiles_for(plan, Fin, Fout, K) != nullptr;
}

static size_t wgrad_slab_bytes(const dsph_plan* plan, const FusedTiles& ft, int32_t Fin, int32_t K) {
  const int C = (Fin + FUSED_CH - 1) / FUSED_CH;
  // (a slab per workgroup and pixel half; a small map's batch is split over up to num_cu workgroups in all: fused_wgrad_gy)
  return (size_t)2 * std::max(fused_grid(plan, ft.ntiles), plan->fused->num_cu) * C * K * 16 * 64 * sizeof(float);
}
size_t fused_wgrad_workspace_bytes(const dsph_plan* plan, int32_t Fin, int32_t Fout, int32_t K) {
  const FusedTiles* ft = wgrad_tiles_for(plan, Fin, Fout, K);
  return ft ? wgrad_slab_bytes(plan, *ft, Fin, K) : 0;
}


// Weight gradient of one 64-column block on the BFS-tile kernel: per-workgroup partial sums into the slabs, then the reduction
// into dw.  rq.only_tiles: the kernel runs on these tiles instead of every tile of the plan (the quad-strip gradient has the others).
static int wgrad_block(const FusedRequest& rq, const FusedTiles* ft, const float* dy, float* dw, float* slabs) {
  const int rc0 = check_request(rq, ft, 0, 0, slabs);
  if (rc0 != DSPH_OK) return rc0;
  const Route rt = make_route(rq.plan, *ft, rq, false);
  FusedArgs args = fused_args(rq, rt);
  args.dy = dy;
  args.slabs = slabs;
  args.y = slabs;  // (nothing is stored through it in this mode)
  if (args.ntiles == 0) return DSPH_OK;
  const int C = args.nchunks, NB = (rq.Fout + 31) / 32, prec = bfs_arithmetic(rq.precision);
  const size_t lds = (size_t)2 * rt.pr * FUSED_CH * 4;
  const int grid = fused_grid(rq.plan, rq.only_tiles ? args.ntiles : ft->ntiles);
  // as many slices per launch as fit the wave's WG_TILES accumulator tiles; every launch runs the
  // recurrence for its own slices only, so the split costs nothing but a second read of dy
  const int per = wgrad_slices_per_launch(*ft, rq.K);
  for (int c0 = 0; c0 < C; c0 += per) {
    FusedArgs la = args;
    la.c_begin = c0;
    la.c_count = std::min(per, C - c0);
    const int rc = launch_fused_variant(rt.pr, ft->width, la, NB, prec, grid, lds, rq.stream);
    if (rc != DSPH_OK) return rc;
  }
  // (Fin_w < Fin: x is a zero-padded copy, only the rows of the real channels exist in dw)
  const int total = rq.Fin_w * rq.K * rq.Fout;
  hipLaunchKernelGGL(fused_wgrad_reduce_kernel, dim3((total + 15) / 16), dim3(256), 0, rq.stream, slabs, dw,
                     2 * grid * fused_wgrad_gy(args.N, grid, args.num_cu), (int)rq.Fin_w, (int)rq.Fout, (int)rq.K, C, (int)rq.ld,
                     prec == DSPH_PREC_BF16X3 ? grid : 0);
  DSPH_HIP(hipGetLastError());
  return DSPH_OK;
}

int launch_cheb_fused_wgrad(const dsph_plan* plan, const float* x, const float* dy, float* dw, int64_t N,
                            int32_t Fin, int32_t Fout, int32_t K, int32_t precision, float alpha_rest, float beta_rest,
                            void* workspace, size_t workspace_bytes, hipStream_t stream, int32_t Fin_w) {
  const FusedTiles* ft = wgrad_tiles_for(plan, Fin, Fout, K);
  if (!ft) {
    set_error("cheb_fused_wgrad: plan/shape not supported");
    return DSPH_E_UNSUPPORTED;
  }
  const size_t need = wgrad_slab_bytes(plan, *ft, Fin, K);
  if (!workspace || workspace_bytes < need) {
    set_error("cheb_fused_wgrad: workspace %zu < %zu", workspace_bytes, need);
    return DSPH_E_WORKSPACE;
  }
  FusedRequest rq;
  rq.mode = Mode::wgrad;
  rq.plan = plan; rq.x = x; rq.stream = stream;
  rq.N = N; rq.Fin = Fin; rq.Fin_w = Fin_w <= 0 ? Fin : Fin_w; rq.ld = Fout; rq.K = K; rq.precision = precision;
  rq.alpha_rest = alpha_rest; rq.beta_rest = beta_rest;
  for (int32_t cb = 0; cb < Fout; cb += 64) {
    rq.Fout = std::min<int32_t>(64, Fout - cb);
    const int rc = wgrad_block(rq, ft, dy + cb, dw + cb, static_cast<float*>(workspace));
    if (rc != DSPH_OK) return rc;
  }
  return DSPH_OK;
}

// ---- quad-strip weight gradient (cheb_qwgrad.hip) -----------------------------------------------------------------------

// The quad-strip weight gradient takes the strips' pixels of a K = 5, 64 -> 64 j layer in the three-term bf16 arithmetic when
// the forward of that shape would run on the quad strips (same tables, same route: that of an unpadded, aligned, whole-map
// forward of one 64-column block) and L~ is symmetric; the BFS-tile kernel's weight-gradient mode takes the tiles the strips
// leave over.
bool fused_qwgrad_applies(const dsph_plan* plan, int64_t N, int32_t Fin, int32_t Fout, int32_t K, int32_t precision) {
  if (precision != DSPH_PREC_BF16X3 || !qwgrad_shape_ok(Fin, 64, K) || Fout % 64 != 0) return false;
  if (!plan->fused || plan->fused->wide || plan->n_rows != plan->n_cols || !plan->levels.empty()) return false;
  if (!fused_wgrad_supported(plan, Fin, Fout, K)) return false;
  const FusedTiles& ft = get_tiles(plan, K - 1, false);
  FusedRequest q;
  q.N = N; q.Fin = q.Fin_w = Fin; q.Fout = 64; q.ld = Fout; q.K = K; q.precision = DSPH_PREC_BF16X3;
  if (!ft.ok || make_route(plan, ft, q, false).strips != Strips::quad) return false;
  return fused_symmetric(plan);
}

size_t fused_qwgrad_workspace_bytes(const dsph_plan* plan) { return qwgrad_slab_bytes(plan->fused ? plan->fused->num_cu : 256); }

// workspace: [the BFS-tile kernel's slabs (fused_wgrad_workspace_bytes, 256-aligned) | the quad strips' slabs]
int launch_cheb_fused_qwgrad(const dsph_plan* plan, const float* x, const float* dy, float* dw, int64_t N, int32_t Fin, int32_t Fout,
                             int32_t K, float alpha_rest, float beta_rest, void* workspace, size_t bfs_slab_bytes, hipStream_t stream) {
  const FusedTiles& ft = get_tiles(plan, K - 1, false);
  const FusedTiles* full = ft.nonq.n > 0 ? tiles_for(plan, Fin, 64, K, true) : nullptr;  // (the BFS-tile kernel's own tables)
  FusedRequest rq;  // (of the BFS-tile kernel's share)
  rq.mode = Mode::wgrad;
  rq.plan = plan; rq.x = x; rq.stream = stream;
  rq.N = N; rq.Fin = rq.Fin_w = Fin; rq.Fout = 64; rq.ld = Fout; rq.K = K; rq.precision = DSPH_PREC_BF16X3;
  rq.alpha_rest = alpha_rest; rq.beta_rest = beta_rest;
  rq.only_tiles = &ft.nonq;
  for (int32_t cb = 0; cb < Fout; cb += 64) {
    if (ft.nonq.n > 0) {
      const int rc = wgrad_block(rq, full, dy + cb, dw + cb, static_cast<float*>(workspace));
      if (rc != DSPH_OK) return rc;
    }
    QWgradLaunch q;
    q.x = x; q.dy = dy + cb; q.dw = dw + cb;
    q.slabs = reinterpret_cast<float*>(static_cast<char*>(workspace) + bfs_slab_bytes);
    q.strips = ft.q5.d_strips; q.prefix = ft.q5.d_prefix; q.tape_rows = ft.q5.tape_rows; q.tab = ft.q5.d_tab;
    q.gvals8 = plan->fused->d_gvals8; q.gdiag = plan->fused->d_gdiag;
    q.x_rows = plan->n_cols; q.dy_rows = plan->n_rows; q.N = N;
    q.nstrips = ft.q5.n; q.lddy = Fout; q.lddw = Fout; q.num_cu = plan->fused->num_cu;
    q.cheb = beta_rest != 0.f;
    q.accumulate = ft.nonq.n > 0;
    const int rc = launch_cheb_qwgrad(q, stream);
    if (rc != DSPH_OK) return rc;
  }
  return DSPH_OK;
}

}  // namespace dsph
