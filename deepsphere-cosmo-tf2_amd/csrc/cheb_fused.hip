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
// Data layout (device):
//   region_rows[tile_off[t] ..]   row ids of tile t's region, ring 0 (the tile's own rows, in
//                                 order) first, then ring 1, ... ring D, each ring ordered so that
//                                 (local index & 3) == (row id & 3) where the ring's mix allows
//   ring_end[t][r]                number of region entries within r hops (r = 0..D)
//   lcols/lvals                   tile-local ELL of the rows within D-1 hops, column = index into
//                                 the region list (uint16), stored [slot][row] per tile so that
//                                 lane i reads row i coalesced
// LDS: two planes [Rmax][16] fp32 (16-byte slots XOR-swizzled so that 16 lanes reading the same
// slot of 16 different rows hit 16 different bank groups) + the weight fragments of all
// (order, slice) pairs in MFMA operand order.
// Registers: each lane owns one (or two) region rows for the whole tile: their ELL values and
// pre-swizzled LDS addresses stay in VGPRs across all slices and all maps of the batch.
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
static size_t wfrag_bytes(int32_t Fin, int32_t Fout, int32_t K) {
  const int C = (Fin + FUSED_CH - 1) / FUSED_CH, NB = bfs_packs(Fin, Fout) ? 2 : (Fout + 31) / 32;
  return (size_t)K * C * NB * 2048;
}

// weight images of the three fused kernels, back to back in the workspace: BFS-tile | structured-tile | strip
static size_t all_frag_bytes(int32_t Fin, int32_t Fout, int32_t K) {
  return wfrag_bytes(Fin, Fout, K) + struct_wfrag_bytes(Fin, Fout, K) + strip_wimg_bytes(Fin, Fout, K) +
         2 * istrip_wimg_bytes(K, DSPH_PREC_BF16X6) +  // (the largest of the three arithmetics, two 32-column blocks)
         (qstrip_shape_ok(Fin, Fout, K) ? qstrip_wimg_bytes() : 0) + (qstrip8_shape_ok(Fin, Fout, K) ? qstrip8_wimg_bytes() : 0);
}

// The structured-tile kernel addresses x by 32-bit byte offsets inside a map: larger maps take BFS tables throughout.
static bool want_full(const dsph_plan* plan, int32_t Fin, bool full) {
  return full || (uint64_t)plan->n_cols * (uint64_t)Fin * 4ull >= (1ull << 32);
}

static bool supported_impl(const dsph_plan* plan, int32_t Fin, int32_t Fout, int32_t K, bool full) {
  full = want_full(plan, Fin, full);
  if (!plan->fused || plan->fused->wide) return false;
  if (K < 2 || K - 1 > FUSED_DMAX) return false;
  if (Fin % 4 != 0 || Fin < 4 || Fout < 1) return false;  // Fout > 64: one launch per 64-column block
  const FusedTiles& ft = get_tiles(plan, K - 1, full);
  if (!ft.ok) return false;
  if (ft.r.n + ft.t.tiles.n > 0 && !struct_shape_ok(Fin, std::min(Fout, 64), K)) return false;
  if (ft.part.n == 0) return true;  // every tile is class R
  const int pr = plane_rows_for(ft.rmax, ft.emax, ft.width);
  if (pr == 0) return false;
  // (the weight fragments need not fit beside the planes: the forward then reads them from global memory, cheb_fused_kernel's
  // WG variant; the planes and weight-gradient modes hold no weights)
  return (size_t)2 * pr * FUSED_CH * 4 + FUSED_BIAS_BYTES <= (size_t)LDS_BYTES;
}

// The forward takes any Fin >= 1: channel counts that are not a multiple of four are zero-padded into the workspace first
// (fused_pad_kernel; the kernels load x in 16-byte pieces).  The first layer of every reference model has Fin = 1.
static inline int32_t pad4(int32_t Fin) { return (Fin + 3) & ~3; }

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

bool fused_supported(const dsph_plan* plan, int32_t Fin, int32_t Fout, int32_t K) {
  return Fin >= 1 && supported_impl(plan, pad4(Fin), Fout, K, false);
}

// ... and with the BFS-tile kernel's weight fragments resident in the LDS (its fast variant: what "supported" meant before the
// WG variant existed; the K > 5 routing of dsphere_api.hip prefers the chain of passes to the WG variant)
bool fused_weights_resident(const dsph_plan* plan, int32_t Fin, int32_t Fout, int32_t K) {
  if (!fused_supported(plan, Fin, Fout, K)) return false;
  const int32_t Fp = pad4(Fin);
  const FusedTiles& ft = get_tiles(plan, K - 1, want_full(plan, Fp, false));
  if (ft.part.n == 0) return true;
  const int pr = plane_rows_for(ft.rmax, ft.emax, ft.width);
  return (size_t)2 * pr * FUSED_CH * 4 + wfrag_bytes(Fp, std::min(Fout, 64), K) + FUSED_BIAS_BYTES <= (size_t)LDS_BYTES;
}

int fused_prepare(const dsph_plan* plan, int32_t K, int32_t Fin, int32_t flags) {
  FusedPlan* fp = plan->fused;
  if (fp && fp->wide) {  // the tiled step's tables, so that the first forward does not build them
    TStepTables tb;
    if (K >= 2) (void)fused_tstep_tables(plan, &tb);
  } else {
    if (!fp || K < 2 || K - 1 > FUSED_DMAX) return DSPH_OK;  // nothing to build: the unfused path serves it
    const FusedTiles& ftp = get_tiles(plan, K - 1, want_full(plan, pad4(std::max(Fin, 1)), false));
    if (ftp.ok && plan->opt.fork && ftp.r.n + ftp.t.tiles.n > 0 && ftp.part.n > 0) {  // a forward of this K may fork: the side stream exists before it
      std::lock_guard<std::mutex> lock(fp->fork_mu);
      (void)side_stream_ready(plan, fp, nullptr, true);
    }
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

// One rule for "does the strip kernel take this forward" (launch_fused_common and dsph_plan_strip_tiles): the shape is the
// kernel's, and the strips are worth it for this batch.  A strip step (48 output pixels of one row, one map) takes a workgroup
// ~3.0 us, a 256-pixel tile of one map takes the tile kernels ~18.7 us of a CU (both measured at the headline shape): in units
// of 0.1 us,   strips: (steps of the busiest workgroup, strip_makespan) x 30      tile kernels: tiles x N x 187 / CUs,
// with 3 % in favour of the tile kernels.  Small maps (fewer items than CUs) and ragged masks at small batches lose that
// comparison and keep their tiles on the tile kernels.  The rule depends on the batch and on the device's CU count, so the
// same map can be summed in two different orders at two batch sizes (both within the tolerance of the precision); a caller
// that needs batch- or shard-invariant bits fixes the choice per plan: dsph_plan_set_option(DSPH_OPT_STRIPS, 1 always | 2 never).
//   Fout: the columns of THIS launch (one 64-column block of the layer); ld: the layer's row stride of y.
static bool use_qstrips(const dsph_plan* plan, const FusedTiles& ft, int32_t Fin, int32_t Fout, int32_t K) {
  return plan->opt.strip_form == 0 && ft.q5.n > 0 && qstrip_shape_ok(Fin, Fout, K);
}
static bool strips_apply(const dsph_plan* plan, const FusedTiles& ft, int32_t Fin, int32_t Fout, int32_t K, int32_t precision, int64_t N,
                         int32_t ld) {
  const bool quad = use_qstrips(plan, ft, Fin, Fout, K);
  if (!((quad || ft.n_pairs > 0) && (precision == DSPH_PREC_BF16X3 || (precision == DSPH_PREC_F16X3 && quad)) &&
        strip_shape_ok(Fin, Fout, K) && ld % 4 == 0 && plan->n_cols * (int64_t)std::max(Fin, ld) * 4 < (1ll << 32)))
    return false;
  if (ft.strip_forced) return true;
  FusedPlan* fp = plan->fused;
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
static bool q8_applies(const dsph_plan* plan, const FusedTiles& ft, int32_t Fin, int32_t Fout, int32_t K, int32_t precision, int64_t N,
                       int32_t ld) {
  // (no limit on the size of a map: this kernel forms its addresses in 64 bits -- configs[3] is 6.4 GB of x)
  // (ld == Fout: the layer IS 32 columns wide -- the last 32 columns of a wider layer would find no room for this kernel's weight
  // image in their block of the workspace, which is sized for 64-column blocks)
  if (ft.q8.n == 0 || !qstrip8_shape_ok(Fin, Fout, K) || (precision != DSPH_PREC_BF16X3 && precision != DSPH_PREC_F16X3) || ld != Fout || N < 1) return false;
  if (plan->opt.strips == 1) return true;
  const int64_t span = qstrip8_split(plan->fused->num_cu, ft.q8.tape_rows, N, ft.q8.tape_rows / std::max(1, ft.q8.n), nullptr, nullptr, nullptr);
  return span * 26 * 103 < ft.q8.n_tiles * N * 275 / plan->fused->num_cu * 100;
}

// The input-side strip kernel takes the rectangles of every layer with at most 16 input channels (any arithmetic, K = 2 .. 5,
// any output width), unless DSPH_OPT_STRIPS says never.  No cost rule: its workers are single waves and the kernel cuts the
// strips into as many row segments as the batch needs, so small maps fill the device too (istrip_segments).
static bool istrips_apply(const dsph_plan* plan, const FusedTiles& ft, int32_t Fin, int32_t K, int32_t Fout, int32_t ld) {
  return ft.n_ipairs > 0 && plan->opt.strips != 2 && istrip_shape_ok(Fin, K) && Fout % 4 == 0 && ld % 4 == 0;
}
static int istrip_nseg(const dsph_plan* plan, const FusedTiles& ft, int64_t N, int D, bool narrow) {
  FusedPlan* fp = plan->fused;
  std::lock_guard<std::mutex> lock(fp->mu);
  const int64_t key = 2 * N + (narrow ? 1 : 0);
  auto it = ft.iseg.find(key);
  if (it == ft.iseg.end()) it = ft.iseg.emplace(key, istrip_segments(ft.ipair_h, ft.ipair_second, N, fp->num_cu, D, narrow)).first;
  return it->second;
}

// conv + HealpyPool(p = 1) in one forward (launch_cheb_fused with a FusedPool): the input-side strip kernels, the structured
// kernel and the BFS-tile kernel store the pooled map themselves.  Every layer whose tiles those kernels take -- not the
// 64 -> 64 shape on maps large enough for the Clenshaw strips --, whole unsharded maps of whole tiles,
// a width that is a multiple of four, bias and ReLU only (the other activations run as a separate pass over the full-resolution map).
bool fused_pool_ok(const dsph_plan* plan, int64_t N, int32_t Fin, int32_t Fout, int32_t K, int32_t act) {
  if (!plan->fused || N < 1 || !(act == DSPH_ACT_NONE || act == DSPH_ACT_RELU)) return false;
  if (!plan->levels.empty() || plan->n_cols != plan->n_rows || plan->n_rows % FUSED_P != 0 || K < 2 || K - 1 > FUSED_DMAX) return false;
  if (!fused_supported(plan, Fin, Fout, K)) return false;
  const FusedTiles& ft = get_tiles(plan, K - 1, want_full(plan, pad4(Fin), false));
  if (!ft.ok || Fout % 4 != 0) return false;  // (pooled stores are 16 bytes wide)
  // the Clenshaw strip kernel has no pooled epilogue: not where it would take tiles (either precision could be asked for)
  return !strips_apply(plan, ft, pad4(Fin), std::min(Fout, 64), K, DSPH_PREC_BF16X3, N, Fout);
}


// tiles a forward of this shape hands to the strip kernel: the same predicate the launch uses, for the layer's first 64-column
// block (a layer with Fout = 96 runs its first block through the strips and reports them; one with Fout < 64 has none)
int64_t fused_strip_tiles(const dsph_plan* plan, int64_t N, int32_t Fin, int32_t Fout, int32_t K, int32_t precision) {
  if (!plan->fused || K < 2 || K - 1 > FUSED_DMAX) return 0;
  if (istrip_shape_ok(pad4(Fin), K)) {
    const FusedTiles& fti = get_tiles(plan, K - 1, want_full(plan, pad4(Fin), false));
    return fti.ok && istrips_apply(plan, fti, pad4(Fin), K, std::min(Fout, 64), Fout) ? fti.n_strip_tiles : 0;
  }
  if (qstrip8_shape_ok(Fin, Fout, K)) {
    const FusedTiles& ft8 = get_tiles(plan, K - 1, want_full(plan, Fin, false));
    return ft8.ok && q8_applies(plan, ft8, Fin, Fout, K, precision, N, Fout) ? ft8.q8.n_tiles : 0;
  }
  if (Fin != pad4(Fin) || Fout < 64) return 0;
  const FusedTiles& ft = get_tiles(plan, K - 1, want_full(plan, Fin, false));
  if (!ft.ok) return 0;
  return strips_apply(plan, ft, Fin, 64, K, precision, N, Fout) ? (use_qstrips(plan, ft, Fin, 64, K) ? ft.q5.n_tiles : ft.n_strip_tiles) : 0;
}

// two fragment layouts: the BFS-tile kernel's and, behind it, the structured-tile kernel's
// (one fragment area per 64-column block of the layer, so that the packed images of ALL blocks survive the call:
// DSPH_FWD_KEEP_WEIGHTS)
static size_t frag_area_bytes(int32_t Fp, int32_t Fout, int32_t K) {
  return (size_t)((Fout + 63) / 64) * all_frag_bytes(Fp, std::min(Fout, 64), K);
}
size_t fused_workspace_bytes(const dsph_plan* plan, int64_t N, int32_t Fin, int32_t Fout, int32_t K, int32_t) {
  const int32_t Fp = pad4(Fin);
  const size_t frag = frag_area_bytes(Fp, Fout, K);
  return frag + (Fp != Fin ? (size_t)N * (size_t)plan->n_cols * (size_t)Fp * 4 : 0);  // + the zero-padded copy of x
}

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

// ------------------------------------------------------------------------------------------
// weight preparation + launch
// ------------------------------------------------------------------------------------------

// Weight fragments in MFMA operand order, one 2 KiB block per (order k, slice c, column block nb):
//   bf16x3: lane l, element j  <- w[(c*16 + 8*(l>>5) + j)*K + k][32*nb + (l&31)], hi at +0, lo at +1024
//   fp32  : step t, lane l     <- w[(c*16 + 8*(l>>5) + t)*K + k][32*nb + (l&31)] at t*256 + l*4
// pack (four maps per item, FusedArgs::pack): one slice, two column blocks, block diagonal -- inner index 4 q + c against columns
// 16 q + o holds w[c*K + k][o].
__global__ __launch_bounds__(256) void fused_wprep_kernel(const float* __restrict__ w,
                                                          unsigned char* __restrict__ out, int Fin,
                                                          int Fout, int K, int C, int NB, int prec, int ld, int pack) {
  const int blk = blockIdx.x;  // (k*C + c)*NB + nb
  const int nb = blk % NB, c = (blk / NB) % C, k = blk / (NB * C);
  for (int e = threadIdx.x; e < 512; e += 256) {
    const int l = e >> 3, j = e & 7;
    const int ch = c * FUSED_CH + 8 * (l >> 5) + j, col = 32 * nb + (l & 31);
    float v;
    if (pack) {  // pack = P maps: 16 / P inner indices and 64 / P columns each
      const int ci = 16 / pack, cm = 64 / pack;
      v = (ch / ci == col / cm && ch % ci < Fin && col % cm < Fout) ? w[((int64_t)(ch % ci) * K + k) * ld + col % cm] : 0.f;
    }
    else v = (ch < Fin && col < Fout) ? w[((int64_t)ch * K + k) * ld + col] : 0.f;
    unsigned char* base = out + (size_t)blk * 2048;
    if (prec == DSPH_PREC_BF16X3) {
      const __bf16 hi = (__bf16)v;
      const __bf16 lo = (__bf16)(v - (float)hi);
      reinterpret_cast<__bf16*>(base)[l * 8 + j] = hi;
      reinterpret_cast<__bf16*>(base + 1024)[l * 8 + j] = lo;
    } else {
      reinterpret_cast<float*>(base)[j * 64 + l] = v;
    }
  }
}

// Diagnostic build only (make ABLATE=1): DSPH_DBG_ONLY=s / b launches only the structured-tile / only the BFS-tile kernel
// (wrong results by construction: the other tiles of y stay unwritten).  The shipped library always launches both.
static inline bool dbg_only(char which) {
#ifdef DSPH_ABLATE
  const char* e = getenv("DSPH_DBG_ONLY");
  return e && e[0] == which;
#else
  (void)which;
  return false;
#endif
}

static int launch_fused_common(const dsph_plan* plan, const float* x, const float* w, const float* bias,
                               float* y, float* planes_out, int64_t N, int32_t Fin, int32_t Fout, int32_t K,
                               int32_t act, int32_t precision, float alpha_rest, float beta_rest,
                               void* workspace, size_t workspace_bytes, hipStream_t stream,
                               const float* dy = nullptr, float* dw = nullptr, int32_t ld = 0, int32_t part = 0,
                               int32_t Fin_w = 0, int32_t only = 0,  // only: 0 every launch, 1 the structured ones, 2 the BFS-tile one
                               bool keep_weights = false,            // the weight images in the workspace are those of an earlier call
                               const FusedPool* pool = nullptr,      // conv + pool: the strips store the pooled map (launch_cheb_fused)
                               const int32_t* wg_tiles = nullptr, int wg_ntiles = -1);  // weight-gradient mode on these tiles only

int launch_cheb_fused(const dsph_plan* plan, const float* x, const float* w, const float* bias,
                      float* y, int64_t N, int32_t Fin, int32_t Fout, int32_t K, int32_t act,
                      int32_t precision, float alpha_rest, float beta_rest, void* workspace,
                      size_t workspace_bytes, hipStream_t stream, int32_t part, bool keep_weights, const FusedPool* pool) {
  if (pool != nullptr && !(part == 0 && fused_pool_ok(plan, N, Fin, Fout, K, act) && pool->y != nullptr && (pool->type == 1 || pool->type == 2) &&
                           ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(pool->y)) & 15) == 0)) {
    set_error("cheb_fused: this plan / shape has no fused pooling (whole unsharded maps, no or ReLU activation, not the Clenshaw strips' shape)");
    return DSPH_E_UNSUPPORTED;
  }
  // more than 64 output columns: one launch per 64-column block (the recurrence is repeated; still one pass
  // over x per block instead of the unfused path's K planes through HBM)
  // The structured-tile kernel fuses bias and ReLU; with any other activation both fused kernels write the pre-activation
  // and one elementwise pass finishes y (only when class-R tiles exist: the BFS-tile kernel knows every activation).
  bool defer_act = false;
  if (act != DSPH_ACT_NONE && act != DSPH_ACT_RELU && K - 1 <= FUSED_DMAX && K >= 2) {
    const FusedTiles& ft = get_tiles(plan, K - 1, want_full(plan, pad4(Fin), false));
    defer_act = ft.ok && ft.r.n + ft.t.tiles.n > 0;
  }
  // (two-part launches: each part writes the pre-activation of its tiles and then finishes exactly those tiles' rows)
  // Fin not a multiple of four: a zero-padded copy of x behind the weight fragments in the workspace (with a two-part
  // launch both parts copy: the halo rows arrive between them)
  const int32_t Fin_w = Fin;
  if (Fin != pad4(Fin)) {
    const int32_t Fp = pad4(Fin);
    const size_t frag = frag_area_bytes(Fp, Fout, K);
    const size_t need = frag + (size_t)N * (size_t)plan->n_cols * (size_t)Fp * 4;
    if (!workspace || workspace_bytes < need) {
      set_error("cheb_fused: workspace %zu < %zu", workspace_bytes, need);
      return DSPH_E_WORKSPACE;
    }
    float* xp = reinterpret_cast<float*>(static_cast<unsigned char*>(workspace) + frag);
    const int rc = launch_fused_pad(x, xp, N * plan->n_cols, Fin, Fp, stream);
    if (rc != DSPH_OK) return rc;
    x = xp;
    Fin = Fp;
  }
  // structured launches and the BFS-tile launch write disjoint tiles: when a forward has both, the latter goes to the plan's
  // side stream (FusedPlan::side), forked behind whatever the caller's stream holds so far and joined before this call returns
  FusedPlan* fp = plan->fused;
  bool fork = false;
  if (fp && plan->opt.fork && K >= 2 && K - 1 <= FUSED_DMAX) {
    const FusedTiles& ft = get_tiles(plan, K - 1, want_full(plan, Fin, false));
    const int ng = !ft.ok ? 0 : ft.part.count(part);
    // (worth its two event operations only when the structured launches run for a while: two tile-maps per CU and more --
    // BASELINE configs[0], 168 tile-maps, is 13 us faster without it, configs[1] 29 us faster with it.  Under a stream
    // capture the fork and the join are edges of the graph and cost nothing at replay: every forward with both kinds of tiles
    // forks there, provided the side stream exists already -- dsph_plan_prepare made it)
    bool big = N * (int64_t)(ft.r.n + ft.t.tiles.n) >= 2 * (int64_t)fp->num_cu;
    if (!big && fp->side && stream != nullptr) {
      hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
      big = hipStreamIsCapturing(stream, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive;
    }
    fork = ft.ok && ft.r.n + ft.t.tiles.n > 0 && ng > 0 && big;
  }
  const size_t blk_frag = all_frag_bytes(Fin, std::min(Fout, 64), K);
  if (!workspace || workspace_bytes < frag_area_bytes(Fin, Fout, K)) {
    set_error("cheb_fused: workspace %zu < %zu", workspace_bytes, frag_area_bytes(Fin, Fout, K));
    return DSPH_E_WORKSPACE;
  }
  for (int32_t cb = 0; cb < Fout; cb += 64) {
    unsigned char* blk_ws = static_cast<unsigned char*>(workspace) + (size_t)(cb / 64) * blk_frag;  // this block's weight images
    fused_images_begin(plan, blk_ws, fused_images_key(Fin, Fin_w, std::min<int32_t>(64, Fout - cb), K, Fout, precision, beta_rest != 0.f,
                                                      N >= 2, plan->opt.pack), keep_weights);
    const FusedPool pool_blk{pool ? pool->y + cb : nullptr, pool ? pool->type : 0};  // (this block's columns of the pooled map)
    const FusedPool* pool_b = pool ? &pool_blk : nullptr;
    auto run = [&](hipStream_t st, int32_t only) {
      return launch_fused_common(plan, x, w + cb, bias ? bias + cb : nullptr, y + cb, nullptr, N, Fin,
                                 std::min<int32_t>(64, Fout - cb), K, defer_act ? DSPH_ACT_NONE : act, precision, alpha_rest,
                                 beta_rest, blk_ws, blk_frag, st, nullptr, nullptr, Fout, part, Fin_w, only, keep_weights, pool_b);
    };
    if (fork) {
      std::unique_lock<std::mutex> lock(fp->fork_mu);
      if (side_stream_ready(plan, fp, stream, true)) {
        DSPH_HIP(hipEventRecord(fp->ev_fork, stream));             // (nothing is on the side stream yet: a failure here or in the
        DSPH_HIP(hipStreamWaitEvent(fp->side, fp->ev_fork, 0));    //  next line leaves nothing to join)
        const int rc_b = run(fp->side, 2);
        const hipError_t e_rec = hipEventRecord(fp->ev_join, fp->side);
        const int rc_s = run(stream, 1);
        // the join happens whatever went wrong in between: the side stream never outlives the call.  (Without the join
        // event the only way to join is to wait for the side stream on the host -- not while the caller is capturing, where
        // a synchronisation would invalidate the capture: the error goes back instead, the capture is lost either way.)
        hipError_t e_join = hipSuccess;
        if (e_rec == hipSuccess) e_join = hipStreamWaitEvent(stream, fp->ev_join, 0);
        else {
          hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
          if (hipStreamIsCapturing(stream, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone) e_join = hipStreamSynchronize(fp->side);
        }
        if (rc_b != DSPH_OK || rc_s != DSPH_OK) fused_images_forget(plan, blk_ws);
        if (rc_b != DSPH_OK) return rc_b;
        if (rc_s != DSPH_OK) return rc_s;
        if (e_rec != hipSuccess) return hip_fail(e_rec, "hipEventRecord(join)");
        if (e_join != hipSuccess) return hip_fail(e_join, "join of the side stream");
        continue;
      }
    }
    const int rc = run(stream, 0);
    if (rc != DSPH_OK) { fused_images_forget(plan, blk_ws); return rc; }
  }
  if (pool != nullptr) {
    return DSPH_OK;  // (every kernel has stored its tiles pooled; y, the scratch of the C ABI, stays untouched)
  }
  if (defer_act) {
    const int64_t orows = plan->levels.empty() ? plan->n_rows : plan->levels[0];
    if (part == 0) return launch_struct_act(y, N * orows, Fout, Fout, act, stream);
    // a part finishes the rows of its own tiles only: INTERIOR and BOUNDARY can be issued in any order, repeated, or alone
    const FusedTiles& ft = get_tiles(plan, K - 1, want_full(plan, Fin, false));
    return launch_struct_act_tiles(y, ft.all.ptr(part), ft.all.count(part), N, orows, Fout, Fout, act, stream);
  }
  return DSPH_OK;
}

// Planes mode of the same kernel: T_1 .. T_{K-1} of x, each (N, n_cols, Fin), valid on the plan's output rows.
bool fused_planes_supported(const dsph_plan* plan, int32_t Fin, int32_t K) { return supported_impl(plan, Fin, 1, K, true); }

int launch_cheb_fused_planes(const dsph_plan* plan, const float* x, float* planes_out, int64_t N, int32_t Fin,
                             int32_t K, float alpha_rest, float beta_rest, hipStream_t stream) {
  return launch_fused_common(plan, x, nullptr, nullptr, nullptr, planes_out, N, Fin, 1, K, DSPH_ACT_NONE,
                             DSPH_PREC_FP32, alpha_rest, beta_rest, nullptr, 0, stream);
}

// ---- weight-gradient mode ------------------------------------------------------------------------------
static int fused_grid(const dsph_plan* plan, const FusedTiles& ft, int ntiles = -1) {
  if (ntiles < 0) ntiles = ft.ntiles;
  return std::max(8, std::min(plan->fused->num_cu, (ntiles + 7) / 8 * 8));
}

// slices per launch: as many accumulator tiles (one per slice and order, 8 KiB each) as fit the LDS next to the planes
static int wgrad_slices_per_launch(const dsph_plan* plan, int32_t K) {
  const FusedTiles& ft = get_tiles(plan, K - 1, true);
  const int pr = plane_rows_for(ft.rmax, ft.emax, ft.width);
  if (pr == 0) return 0;
  const long freeb = (long)LDS_BYTES - 2L * pr * FUSED_CH * 4;
  return (int)(freeb / ((long)K * WG_TILE_BYTES));
}

bool fused_wgrad_supported(const dsph_plan* plan, int32_t Fin, int32_t Fout, int32_t K) {
  return supported_impl(plan, Fin, Fout, K, true) && wgrad_slices_per_launch(plan, K) >= 1;
}

size_t fused_wgrad_workspace_bytes(const dsph_plan* plan, int32_t Fin, int32_t Fout, int32_t K) {
  if (!fused_wgrad_supported(plan, Fin, Fout, K)) return 0;
  const FusedTiles& ft = get_tiles(plan, K - 1, true);
  const int C = (Fin + FUSED_CH - 1) / FUSED_CH;
  // (a slab per workgroup and pixel half; a small map's batch is split over up to num_cu workgroups in all: fused_wgrad_gy)
  return (size_t)2 * std::max(fused_grid(plan, ft), plan->fused->num_cu) * C * K * 16 * 64 * sizeof(float);
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

int launch_cheb_fused_wgrad(const dsph_plan* plan, const float* x, const float* dy, float* dw, int64_t N,
                            int32_t Fin, int32_t Fout, int32_t K, int32_t precision, float alpha_rest, float beta_rest,
                            void* workspace, size_t workspace_bytes, hipStream_t stream, int32_t Fin_w) {
  if (!fused_wgrad_supported(plan, Fin, Fout, K)) {
    set_error("cheb_fused_wgrad: plan/shape not supported");
    return DSPH_E_UNSUPPORTED;
  }
  const size_t need = fused_wgrad_workspace_bytes(plan, Fin, Fout, K);
  if (!workspace || workspace_bytes < need) {
    set_error("cheb_fused_wgrad: workspace %zu < %zu", workspace_bytes, need);
    return DSPH_E_WORKSPACE;
  }
  for (int32_t cb = 0; cb < Fout; cb += 64) {
    const int rc = launch_fused_common(plan, x, nullptr, nullptr, static_cast<float*>(workspace), nullptr, N, Fin,
                                       std::min<int32_t>(64, Fout - cb), K, DSPH_ACT_NONE, precision, alpha_rest,
                                       beta_rest, nullptr, 0, stream, dy + cb, dw + cb, Fout, 0, Fin_w);
    if (rc != DSPH_OK) return rc;
  }
  return DSPH_OK;
}

// ---- quad-strip weight gradient (cheb_qwgrad.hip) -----------------------------------------------------------------------

// The quad-strip weight gradient takes the strips' pixels of a K = 5, 64 -> 64 j layer in the three-term bf16 arithmetic when
// the forward of that shape would run on the quad strips (same tables, same cost rule) and L~ is symmetric; the BFS-tile
// kernel's weight-gradient mode takes the tiles the strips leave over.
bool fused_qwgrad_applies(const dsph_plan* plan, int64_t N, int32_t Fin, int32_t Fout, int32_t K, int32_t precision) {
  if (precision != DSPH_PREC_BF16X3 || !qwgrad_shape_ok(Fin, 64, K) || Fout % 64 != 0) return false;
  if (!plan->fused || plan->fused->wide || plan->n_rows != plan->n_cols || !plan->levels.empty()) return false;
  if (!fused_wgrad_supported(plan, Fin, Fout, K)) return false;
  const FusedTiles& ft = get_tiles(plan, K - 1, false);
  if (!ft.ok || !use_qstrips(plan, ft, Fin, 64, K) || !strips_apply(plan, ft, Fin, 64, K, DSPH_PREC_BF16X3, N, Fout)) return false;
  return fused_symmetric(plan);
}

size_t fused_qwgrad_workspace_bytes(const dsph_plan* plan) { return qwgrad_slab_bytes(plan->fused ? plan->fused->num_cu : 256); }

// workspace: [the BFS-tile kernel's slabs (fused_wgrad_workspace_bytes, 256-aligned) | the quad strips' slabs]
int launch_cheb_fused_qwgrad(const dsph_plan* plan, const float* x, const float* dy, float* dw, int64_t N, int32_t Fin, int32_t Fout,
                             int32_t K, float alpha_rest, float beta_rest, void* workspace, size_t bfs_slab_bytes, hipStream_t stream) {
  const FusedTiles& ft = get_tiles(plan, K - 1, false);
  for (int32_t cb = 0; cb < Fout; cb += 64) {
    if (ft.nonq.n > 0) {
      const int rc = launch_fused_common(plan, x, nullptr, nullptr, static_cast<float*>(workspace), nullptr, N, Fin, 64, K, DSPH_ACT_NONE,
                                         DSPH_PREC_BF16X3, alpha_rest, beta_rest, nullptr, 0, stream, dy + cb, dw + cb, Fout, 0, Fin, 0, false,
                                         nullptr, ft.nonq.d, ft.nonq.n);
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

static int launch_fused_common(const dsph_plan* plan, const float* x, const float* w, const float* bias,
                               float* y, float* planes_out, int64_t N, int32_t Fin, int32_t Fout, int32_t K,
                               int32_t act, int32_t precision, float alpha_rest, float beta_rest,
                               void* workspace, size_t workspace_bytes, hipStream_t stream, const float* dy,
                               float* dw, int32_t ld, int32_t part, int32_t Fin_w, int32_t only, bool keep_weights,
                               const FusedPool* pool, const int32_t* wg_tiles, int wg_ntiles) {
  // DSPH_PREC_F16X3 is the quad strips' arithmetic; every other kernel of the forward runs the six-term split (same accuracy)
  const bool f16 = precision == DSPH_PREC_F16X3;
  const int32_t strip_precision = precision;
  if (f16) precision = DSPH_PREC_BF16X6;
  if (ld <= 0) ld = Fout;
  if (Fin_w <= 0) Fin_w = Fin;  // channels of w; smaller than Fin when x is a zero-padded copy  // row stride of w, bias-less y / dy / dw: the layer's Fout when this is one column block
  const bool wgrad_mode = dy != nullptr;  // y then carries the slab workspace
  const bool planes_mode = planes_out != nullptr || wgrad_mode;
  if (!supported_impl(plan, Fin, Fout, K, planes_mode)) {
    set_error("cheb_fused: plan/shape not supported");
    return DSPH_E_UNSUPPORTED;
  }
  const FusedTiles& ft = get_tiles(plan, K - 1, want_full(plan, Fin, planes_mode));
  const size_t wb = planes_mode ? 0 : wfrag_bytes(Fin, Fout, K);
  const size_t wb_all = planes_mode ? 0 : all_frag_bytes(Fin, Fout, K);
  if (!planes_mode && (!workspace || workspace_bytes < wb_all)) {
    set_error("cheb_fused: workspace %zu < %zu", workspace_bytes, wb_all);
    return DSPH_E_WORKSPACE;
  }
  if ((reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(workspace) & 15) ||
      (reinterpret_cast<uintptr_t>(planes_out) & 15) || (wgrad_mode && (reinterpret_cast<uintptr_t>(y) & 15))) {
    set_error("cheb_fused: x, workspace and planes must be 16-byte aligned");
    return DSPH_E_BADARG;
  }
  const int C = (Fin + FUSED_CH - 1) / FUSED_CH, NB = (Fout + 31) / 32;
  // ---- class-R and class-T tiles: the structured-tile kernel (forward only), without and with per-tile tables ----------
  if (!planes_mode && ft.r.n + ft.t.tiles.n > 0 && only != 2) {
    StructLaunch sl;
    sl.x = x; sl.w = w; sl.bias = bias; sl.y = y;
    sl.wfrag = static_cast<unsigned char*>(workspace) + wb;
    sl.gvals8 = plan->fused->d_gvals8;
    sl.gdiag = plan->fused->d_gdiag;
    sl.x_rows = plan->n_cols;
    sl.y_rows = plan->levels.empty() ? plan->n_rows : plan->levels[0];
    sl.N = N;
    sl.Fin = Fin; sl.Fin_w = Fin_w; sl.Fout = Fout; sl.K = K; sl.act = act; sl.precision = precision; sl.ld = ld;
    sl.num_cu = plan->fused->num_cu;
    sl.cheb = beta_rest != 0.f;
    bool struct_prep = true;  // the first structured launch of this call packs the fragments, if the block lacks them
    sl.allow_pack = plan->opt.pack;
    if (pool != nullptr) {
      sl.pool = pool->type;
      sl.ypool = pool->y;
      sl.ypool_rows = plan->n_rows / 4;
    }
    // rectangles of interior class-R tiles: the strip kernel, when it has this shape; the class-R list shrinks to the rest
    const bool strips = strips_apply(plan, ft, Fin, Fout, K, strip_precision, N, ld) && Fin_w == Fin && (reinterpret_cast<uintptr_t>(y) & 15) == 0;
    if (strips && part != 2 && !dbg_only('b') && use_qstrips(plan, ft, Fin, Fout, K)) {
      QStripLaunch qs;
      qs.x = x; qs.w = w; qs.bias = bias; qs.y = y;
      qs.wimg = static_cast<unsigned char*>(workspace) + wb + struct_wfrag_bytes(Fin, Fout, K) + strip_wimg_bytes(Fin, Fout, K) +
                2 * istrip_wimg_bytes(K, DSPH_PREC_BF16X6);
      qs.strips = ft.q5.d_strips;
      qs.tab = ft.q5.d_tab;
      qs.prefix = ft.q5.d_prefix;
      qs.tape_rows = ft.q5.tape_rows;
      qs.gvals8 = plan->fused->d_gvals8;
      qs.gdiag = plan->fused->d_gdiag;
      qs.x_rows = sl.x_rows; qs.y_rows = sl.y_rows; qs.N = N;
      qs.nstrips = ft.q5.n; qs.Fin = Fin; qs.Fout = Fout; qs.act = act; qs.ld = ld;
      qs.num_cu = plan->fused->num_cu;
      qs.cheb = sl.cheb;
      qs.f16 = f16;
      qs.f16_xexp = plan->opt.f16_xexp;
      qs.prep_weights = fused_images_claim(plan, workspace, IMG_QSTRIP);
      const int rc = launch_cheb_qstrip(qs, stream);
      if (rc != DSPH_OK) return rc;
    } else if (strips && part != 2 && !dbg_only('b')) {
      StripLaunch st;
      st.x = x; st.w = w; st.bias = bias; st.y = y;
      st.wimg = static_cast<unsigned char*>(workspace) + wb + struct_wfrag_bytes(Fin, Fout, K);
      st.pairs = ft.d_pairs;
      st.gvals8 = plan->fused->d_gvals8;
      st.gdiag = plan->fused->d_gdiag;
      st.x_rows = sl.x_rows; st.y_rows = sl.y_rows; st.N = N;
      st.npairs = ft.n_pairs; st.Fin = Fin; st.Fout = Fout; st.K = K; st.act = act; st.precision = precision; st.ld = ld;
      st.num_cu = plan->fused->num_cu;
      st.cheb = sl.cheb;
      st.generic = plan->opt.strip_generic;
      st.prep_weights = fused_images_claim(plan, workspace, IMG_STRIP);
      const int rc = launch_cheb_strip(st, stream);
      if (rc != DSPH_OK) return rc;
    }
    const bool istrips = !strips && istrips_apply(plan, ft, Fin, K, Fout, ld) && (reinterpret_cast<uintptr_t>(y) & 15) == 0;
    if (istrips && part != 2 && !dbg_only('b')) {
      IStripLaunch is;
      is.x = x; is.w = w; is.bias = bias; is.y = y;
      is.wimg = static_cast<unsigned char*>(workspace) + wb + struct_wfrag_bytes(Fin, Fout, K) + strip_wimg_bytes(Fin, Fout, K);
      is.pairs = ft.d_ipairs;
      is.gvals8 = plan->fused->d_gvals8;
      is.gdiag = plan->fused->d_gdiag;
      is.x_rows = sl.x_rows; is.y_rows = sl.y_rows; is.N = N;
      is.npairs = ft.n_ipairs; is.Fin = Fin; is.Fin_w = Fin_w; is.Fout = Fout; is.K = K; is.act = act; is.precision = precision; is.ld = ld;
      is.num_cu = plan->fused->num_cu;
      // (row segments for the items the kernel will deal: maps, or pairs of maps in the one-channel kernel's pair mode)
      is.nseg = istrip_nseg(plan, ft, istrip_pairs(Fin_w, Fout) ? (N + 1) / 2 : N, K - 1, istrip_narrow(Fin_w));
      is.cheb = sl.cheb;
      is.prep_weights = fused_images_claim(plan, workspace, IMG_ISTRIP);
      if (pool != nullptr) {
        is.pool = pool->type;
        is.ypool = pool->y;
        is.ypool_rows = plan->n_rows / 4;
      }
      const int rc = launch_cheb_istrip(is, stream);
      if (rc != DSPH_OK) return rc;
    }
    const bool stripped = strips || istrips;
    const bool qrest = strips && use_qstrips(plan, ft, Fin, Fout, K);  // the quad strips took class-T tiles too: their own rest lists
    const TileList& rl = qrest ? ft.qrrest : (stripped ? ft.rrest : ft.r);
    if (rl.count(part) > 0 && !dbg_only('b')) {
      sl.tiles = rl.ptr(part);
      sl.tabrow = nullptr;
      sl.tabvals = nullptr;
      sl.ntiles = rl.count(part);
      sl.prep_weights = struct_prep && fused_images_claim(plan, workspace, IMG_STRUCT);
      struct_prep = false;
      const int rc = launch_cheb_struct(sl, stream);
      if (rc != DSPH_OK) return rc;
    }
    const TileTables& tt = qrest ? ft.qt : ft.t;
    if (tt.tiles.count(part) > 0 && !dbg_only('b')) {
      sl.tiles = tt.tiles.ptr(part);
      sl.tabrow = tt.rows(part);
      sl.tabvals = tt.vals(part);
      sl.ntiles = tt.tiles.count(part);
      sl.prep_weights = struct_prep && fused_images_claim(plan, workspace, IMG_STRUCT);
      struct_prep = false;
      const int rc = launch_cheb_struct(sl, stream);
      if (rc != DSPH_OK) return rc;
    }
    if (ft.part.count(part) == 0 || dbg_only('s')) return DSPH_OK;
  }
  if (only == 1) return DSPH_OK;
  // the BFS-tile kernel has two contraction arithmetics; the six-term split of the structured kernel is fp32-equivalent
  if (precision == DSPH_PREC_BF16X6) precision = DSPH_PREC_FP32;
  // four maps per item where the layer has at most four input channels and 16 output columns (FusedArgs::pack)
  const int pack = (plan->opt.pack && !planes_mode && !wgrad_mode && N >= 2) ? bfs_packs(Fin, Fout) : 0;  // (a single map gains nothing from two column blocks)
  const int NBb = pack ? 2 : NB;
  if (!planes_mode && fused_images_claim(plan, workspace, IMG_BFS)) {
    hipLaunchKernelGGL(fused_wprep_kernel, dim3(K * C * NBb), dim3(256), 0, stream, w,
                       static_cast<unsigned char*>(workspace), (int)Fin_w, (int)Fout, (int)K, C, NBb,
                       (int)precision, (int)ld, pack);
    DSPH_HIP(hipGetLastError());
  }

  // K = 8, 32 -> 32: the rectangles of depth-7 regular tiles on the quad strips, the rest of the tiles below
  const bool q8 = !planes_mode && part != 2 && pool == nullptr && only == 0 && Fin_w == Fin && beta_rest != 0.f &&
                  (act == DSPH_ACT_NONE || act == DSPH_ACT_RELU) && (reinterpret_cast<uintptr_t>(y) & 15) == 0 &&
                  q8_applies(plan, ft, Fin, Fout, K, strip_precision, N, ld);
  if (q8) {
    QStrip8Launch q;
    q.x = x; q.w = w; q.bias = bias; q.y = y;
    q.wimg = static_cast<unsigned char*>(workspace) + all_frag_bytes(Fin, Fout, K) - qstrip8_wimg_bytes();
    q.strips = ft.q8.d_strips; q.tab = ft.q8.d_tab; q.prefix = ft.q8.d_prefix; q.tape_rows = ft.q8.tape_rows;
    q.gvals8 = plan->fused->d_gvals8; q.gdiag = plan->fused->d_gdiag;
    q.x_rows = plan->n_cols; q.y_rows = plan->levels.empty() ? plan->n_rows : plan->levels[0]; q.N = N;
    q.nstrips = ft.q8.n; q.act = act; q.ld = ld; q.ld_w = ld; q.num_cu = plan->fused->num_cu;
    q.f16 = f16;
    q.f16_xexp = plan->opt.f16_xexp;
    q.prep_weights = fused_images_claim(plan, workspace, IMG_Q8);
    const int rc = launch_cheb_qstrip8(q, stream);
    if (rc != DSPH_OK) return rc;
    if (ft.q8rest.count(part) == 0) return DSPH_OK;
  }

  FusedArgs args;
  args.planes_out = planes_out;
  args.dy = dy;
  args.slabs = wgrad_mode ? y : nullptr;
  args.c_begin = 0;
  args.c_count = C;
  args.prow_stride = plan->n_cols;
  args.plane_stride = N * plan->n_cols * (int64_t)Fin;
  args.x = x;
  args.bias = bias;
  args.y = y;
  args.wfrag = static_cast<const unsigned char*>(workspace);
  args.tile_off = ft.d_tile_off;
  args.ring_end = ft.d_ring_end;
  args.ell_off = ft.d_ell_off;
  args.region = ft.d_region;
  args.lcols = ft.d_lcols;
  args.lvals = ft.d_lvals;
  args.x_rows = plan->n_cols;
  args.y_rows = plan->levels.empty() ? plan->n_rows : plan->levels[0];
  args.N = pack ? (int)((N + pack - 1) / pack) : (int)N;  // (packed: groups of P maps)
  args.n_maps = (int)N;
  args.pack = pack;
  args.num_cu = plan->fused->num_cu;
  args.pool = pool ? pool->type : 0;
  args.ypool = pool ? pool->y : nullptr;
  args.ypool_rows = plan->n_rows / 4;
  args.Fin = Fin;
  args.Fout = Fout;
  args.ld = ld;
  args.K = K;
  // part: 0 all tiles, 1 interior tiles (no row of another rank in their region), 2 boundary tiles
  // the BFS-tile kernel handles the tiles of ft.part (every tile of a full table, the class-G ones otherwise)
  args.tile_list = part == 0 && ft.part.n == ft.ntiles ? nullptr : ft.part.ptr(part);
  args.ntiles = ft.part.count(part);
  if (q8) {  // (part 0: every tile the strips leave; part 1: the interior ones of them -- the boundary tiles are never the strips')
    args.tile_list = ft.q8rest.ptr(part);
    args.ntiles = ft.q8rest.count(part);
  }
  if (wgrad_mode && wg_ntiles >= 0) {  // (the strips' pixels go to cheb_qwgrad.hip: launch_cheb_fused_qwgrad)
    args.tile_list = wg_tiles;
    args.ntiles = wg_ntiles;
  }
  if (args.ntiles == 0) return DSPH_OK;
  args.nchunks = C;
  args.act = act;
  args.alpha_rest = alpha_rest;
  args.beta_rest = beta_rest;
  args.wfrag_bytes = (int)wb;
#ifdef DSPH_ABLATE  // diagnostic build only (make ABLATE=1): the shipped library never skips work
  const char* dbg = getenv("DSPH_FUSED_DEBUG");
  args.dbg = dbg ? atoi(dbg) : 0;
#else
  args.dbg = 0;
#endif
  const int pr = plane_rows_for(ft.rmax, ft.emax, ft.width);
  const size_t lds = (size_t)2 * pr * FUSED_CH * 4 + wb;
  const int grid = (wgrad_mode && wg_ntiles < 0) ? fused_grid(plan, ft) : fused_grid(plan, ft, args.ntiles);
  if (wgrad_mode) {
    // as many slices per launch as fit the wave's WG_TILES accumulator tiles; every launch runs the
    // recurrence for its own slices only, so the split costs nothing but a second read of dy
    const int per = wgrad_slices_per_launch(plan, K);
    for (int c0 = 0; c0 < C; c0 += per) {
      FusedArgs la = args;
      la.c_begin = c0;
      la.c_count = std::min(per, C - c0);
      const int rc = launch_fused_variant(pr, ft.width, la, NB, precision, grid, lds, stream);
      if (rc != DSPH_OK) return rc;
    }
    // (Fin_w < Fin: x is a zero-padded copy, only the rows of the real channels exist in dw)
    const int total = Fin_w * K * Fout;
    hipLaunchKernelGGL(fused_wgrad_reduce_kernel, dim3((total + 15) / 16), dim3(256), 0, stream, args.slabs, dw,
                       2 * grid * fused_wgrad_gy(args.N, grid, args.num_cu), (int)Fin_w, (int)Fout, (int)K, C, (int)ld,
                       precision == DSPH_PREC_BF16X3 ? grid : 0);
    DSPH_HIP(hipGetLastError());
    return DSPH_OK;
  }
#ifdef DSPH_STAMPS
  static unsigned long long* d_stamps = nullptr;
  constexpr size_t NST = 8 * 8 * 32;
  if (!d_stamps) DSPH_HIP(hipMalloc(&d_stamps, NST * 8));
  DSPH_HIP(hipMemsetAsync(d_stamps, 0, NST * 8, stream));
  args.stamps = d_stamps;
  auto dump_stamps = [&](int rc) {
    if (rc != DSPH_OK || !getenv("DSPH_STAMPS_DUMP")) return rc;
    std::vector<unsigned long long> h(NST);
    if (hipStreamSynchronize(stream) != hipSuccess) return rc;
    if (hipMemcpy(h.data(), d_stamps, NST * 8, hipMemcpyDeviceToHost) != hipSuccess) return rc;
    for (int w = 0; w < 8; ++w)
      for (int it = 0; it < 8; ++it) {
        fprintf(stderr, "STAMP wave %d item %d:", w, it + 4);
        const unsigned long long* r = &h[((size_t)w * 8 + it) * 32];
        for (int i = 1; i < 32; ++i) fprintf(stderr, " %lld", r[i] && r[i - 1] ? (long long)(r[i] - r[i - 1]) : -1LL);
        fprintf(stderr, " | t0 %llu\n", r[0]);
      }
    return rc;
  };
  return dump_stamps(launch_fused_variant(pr, ft.width, args, NBb, precision, grid, lds, stream));
#else
  return launch_fused_variant(pr, ft.width, args, NBb, precision, grid, lds, stream);
#endif
}

}  // namespace dsph
