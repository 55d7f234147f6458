/* dsphere.h -- C ABI of the MI355X-native Chebyshev graph-convolution forward.
 *
 * Drop-in boundary for ONE path of deepsphere/deepsphere-cosmo-tf2: the forward of
 * `deepsphere.gnn_layers.Chebyshev` (reference src/deepsphere/gnn_layers.py:106-161) with
 * its one-time Laplacian upload (gnn_layers.py:64-72).  The reference has no FFI of its
 * own for this path -- it calls TensorFlow ops from Python -- so every entry point below
 * names the Python/TF call sites it replaces.  Plain pointers and sizes only; no torch
 * types.  All device pointers are HIP device memory on the plan's device; the caller
 * (PyTorch) owns x, w, bias, y and the workspace.  Functions return 0 on success or a
 * negative DSPH_E_* code; the message is available from dsph_last_error() (thread-local).
 *
 * Allocation and synchronisation: dsph_plan_create, dsph_plan_prepare, dsph_plan_set_levels and
 * dsph_plan_destroy allocate / free device memory and synchronise.  The compute entry points
 * (dsph_cheb_*, dsph_poly_*, dsph_rows_*) only enqueue kernels on the caller's stream -- EXCEPT that
 * the first fused call for a (plan, K) that has not been through dsph_plan_prepare builds the tile
 * tables on the spot (device allocation + synchronous copies).  Call dsph_plan_prepare once per K
 * before timing, and before capturing a forward into a hipGraph; after it, a forward neither
 * allocates nor synchronises (tests/test_gpu_parity.py::test_prepared_forward_*).
 */
#ifndef DSPHERE_H
#define DSPHERE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSPH_ABI_VERSION 3  /* 3: DSPH_OPT_F16_XEXP, dsph_plan_strip_rows, dsph_plan_uses_chain (round 6); 2: dsph_plan_prepare_layer; the entry points added
                              * since version 1 (set_option, forward_ex, forward_pool, healpix_pool, strip_pairs) are part of it;
                              * still 3 without the options 5 and 7: no symbol or struct changed */

/* error codes */
#define DSPH_OK 0
#define DSPH_E_BADARG (-1)      /* null pointer, negative size, inconsistent shapes */
#define DSPH_E_HIP (-2)         /* a HIP runtime call failed */
#define DSPH_E_UNSUPPORTED (-3) /* shape outside what the kernels implement */
#define DSPH_E_WORKSPACE (-4)   /* workspace too small */

/* fused epilogue activations (reference: tf.keras.activations looked up by name,
 * gnn_layers.py:55-60; anything else is applied by the host layer after the call) */
#define DSPH_ACT_NONE 0
#define DSPH_ACT_RELU 1
#define DSPH_ACT_ELU 2
#define DSPH_ACT_SIGMOID 3
#define DSPH_ACT_TANH 4

/* arithmetic of the dense [K*Fin]x[Fout] contraction (the recurrence is always fp32) */
#define DSPH_PREC_FP32 0   /* v_mfma_f32_32x32x2_f32: bitwise an fp32 fma chain        */
#define DSPH_PREC_BF16X3 1 /* hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16, fp32 accumulate */
/* fp32-equivalent on the bf16 matrix pipe: both operands split three ways (8 + 8 + 8 mantissa bits), the six products
 * down to 2^-16 kept (hh, hm, mh, mm, hl, lh), fp32 accumulate: what is dropped is 2^-23 of a product, the size of an
 * fp32 rounding.  A third of the matrix-pipe time of DSPH_PREC_FP32.  The structured-tile kernel implements it; every
 * other kernel (BFS tiles, unfused, weight gradient) runs DSPH_PREC_FP32 when asked for it. */
#define DSPH_PREC_BF16X6 2
/* fp32-equivalent at the three-term split's price, where the quad-strip kernels run (csrc/cheb_qstrip_kernel.h: K = 5, 64 input
 * and 64 output channels per column block; csrc/cheb_qstrip8_kernel.h: K = 8, 32 -> 32; the rectangles of a HEALPix map): both operands split hi + lo into f16 (11 + 11
 * mantissa bits), hi.hi + hi.lo + lo.hi on v_mfma_f32_16x16x32_f16, fp32 accumulate: what is dropped is 2^-22 of a product.
 * The weights go in times a power of two of the library's choosing (taken out again in the store); x goes in times 2^e, e =
 * DSPH_OPT_F16_XEXP of the plan (default 0), taken out again in the store as well.  The RANGE CONDITION is the caller's to meet:
 *   upper: |x| 2^e < 65,504 -- an input beyond it does not fit an f16 and comes out as Inf / NaN rows of y (loud);
 *   lower: an f16 pair keeps 22 bits only where both halves are normal numbers, |x| 2^e >= 2^-3; below that the lo half goes
 *          subnormal and the absolute error of an input element stays at 2^-25 (2^-e of it in x's units): with unit-variance x and e
 *          = 0 the result is 3e-7 of max|y| from float64, with x of scale 1e-3 and e = 0 it is 2e-5 -- WORSE than DSPH_PREC_BF16X3
 *          (silent).  Choose e so that max|x| 2^e lies in [2^13, 2^15): every element within 2^-16 of the maximum then keeps its
 *          22 bits and the smaller ones err by 2^-38 of the maximum (deepsphere/gnn_layers.py does this from `x_absmax`, or
 *          from a reduction over x when the caller names no scale).
 * Every tile, shape and kernel the quad strips do not take runs DSPH_PREC_BF16X6 (same accuracy, no range condition). */
#define DSPH_PREC_F16X3 3

/* polynomial basis of the recurrence: T_1 = L~ x in both;
 *   Chebyshev: T_k = 2 L~ T_{k-1} - T_{k-2}   (reference gnn_layers.Chebyshev, gnn_layers.py:137-143)
 *   monomial:  T_k = L~ T_{k-1}                (reference gnn_layers.Monomial,  gnn_layers.py:283-286) */
#define DSPH_BASIS_CHEBYSHEV 0
#define DSPH_BASIS_MONOMIAL 1

/* which implementation dsph_cheb_forward runs */
#define DSPH_ALGO_AUTO 0
#define DSPH_ALGO_UNFUSED 1 /* K-1 ELL SpMM launches into workspace planes + one contraction launch */
#define DSPH_ALGO_FUSED 2   /* one launch: tile + halo in LDS, planes never leave the CU */

typedef struct dsph_plan dsph_plan;

/* Upload the rescaled Laplacian L~ once.
 * Replaces: the tf.constant triple built in Chebyshev.__init__ (gnn_layers.py:68-72) and the
 * per-call tf.SparseTensor + tf.sparse.reorder (gnn_layers.py:114-115).
 *   n_rows      rows of L~ held by this plan (outputs are produced for rows [0, n_rows))
 *   n_cols      length of the vectors L~ is applied to; n_cols >= n_rows.  Equal for a whole
 *               graph; larger for a shard whose trailing n_cols - n_rows entries are halo rows
 *               received from other shards.
 *   ell_width   padded row width W (max non-zeros per row, diagonal included)
 *   cols, vals  HOST arrays [n_rows][ell_width], row-major; padding entries carry val 0 and any
 *               valid column (conventionally the row itself)
 *   device      HIP device ordinal
 */
int dsph_plan_create(dsph_plan** out, int64_t n_rows, int64_t n_cols, int32_t ell_width,
                     const int32_t* cols, const float* vals, int device);

void dsph_plan_destroy(dsph_plan* plan);

/* Optional shrinking schedule for a plan whose rows are ordered by graph distance from the
 * rows it owns (sharded, deep-halo mode): rows_at_level[j] = number of leading rows within j
 * hops of the owned rows, j = 0..n_levels-1, non-decreasing, rows_at_level[0] = owned rows,
 * rows_at_level[n_levels-1] <= n_rows.  With a schedule, recurrence step k of a K-term forward
 * is evaluated on rows_at_level[K-1-k] rows (so a K-term forward needs n_levels >= K-1) and y
 * is written for rows_at_level[0] rows.  Without one every step covers n_rows rows.
 * Host array, copied. */
int dsph_plan_set_levels(dsph_plan* plan, int32_t n_levels, const int64_t* rows_at_level);

/* Build everything the fused kernels need from this plan for a K-term layer with Fin input channels, now
 * instead of inside the first forward: the direction-ordered copy of L~ and the per-row / per-tile verification
 * of the 2-D stencil structure (structured-tile kernel), and the breadth-first ring tables of the remaining
 * tiles (BFS-tile kernel).  Allocates device memory, launches set-up kernels and synchronises.
 *   flags  DSPH_PREPARE_BACKWARD      also the tables of dsph_cheb_planes / dsph_cheb_backward_weights, and the look at the
 *                                     matrix that dsph_cheb_backward_weights otherwise takes on its first call (is it
 *                                     symmetric: one host pass over the ELL arrays, about a second at 12.6 M rows)
 *          DSPH_PREPARE_RELEASE_HOST  afterwards drop the plan's host copy of the ELL arrays (kept by
 *                                     dsph_plan_create to build tables for further K); preparing another K
 *                                     later then fails with DSPH_E_UNSUPPORTED and forwards with that K take
 *                                     the unfused path under DSPH_ALGO_AUTO; dsph_plan_set_levels then returns
 *                                     DSPH_E_UNSUPPORTED (it would have to rebuild the tables), and the tables of
 *                                     dsph_cheb_planes / dsph_cheb_backward_weights exist only if DSPH_PREPARE_BACKWARD
 *                                     was passed in the same call
 * Returns DSPH_OK also when the fused kernels cannot run the plan (dsph_plan_fused_ok says which). */
#define DSPH_PREPARE_BACKWARD 1
#define DSPH_PREPARE_RELEASE_HOST 2
int dsph_plan_prepare(dsph_plan* plan, int32_t K, int32_t Fin, int32_t flags);
/* The same for a layer whose output width is known: a K > 5 layer runs either on the breadth-first tables of depth K - 1 or as
 * a chain of K <= 5 passes (DSPH_OPT_SPLIT), and which of the two depends on Fin AND Fout; this call builds exactly the tables
 * the forward of (K, Fin, Fout) will use, by the forward's own rule.  dsph_plan_prepare(plan, K, Fin, flags) is this call with
 * Fout = Fin. */
int dsph_plan_prepare_layer(dsph_plan* plan, int32_t K, int32_t Fin, int32_t Fout, int32_t flags);

/* Per-plan choices.  The library reads no environment variable: what used to be process-global switches of the fused path
 * are options of the plan, set before the tables of a K are built (dsph_plan_prepare or the first forward) -- setting one that
 * changes the tables drops the cached ones, like dsph_plan_set_levels, and after DSPH_PREPARE_RELEASE_HOST returns
 * DSPH_E_UNSUPPORTED.  Not thread-safe against forwards in flight on the same plan.
 *   DSPH_OPT_STRIPS         0 (default): whether the strip kernel takes its rectangles is decided per call by a cost rule that
 *                           depends on the batch N and the device's CU count (csrc/cheb_fused.hip, strips_apply) -- so the
 *                           same map on the same plan can be summed in Clenshaw order at one batch size and in forward order
 *                           at another, equal to rounding, not bit for bit; 1: always (when the shape is the kernel's);
 *                           2: never.  1 and 2 make the choice independent of batch, device and sharding.
 *   DSPH_OPT_STRUCT         1 (default) / 0: the structured-tile kernel for tiles that verify as a 2-D stencil; 0 sends
 *                           every tile to the breadth-first-table kernel
 *   DSPH_OPT_TABLES         1 (default) / 0: per-tile tables (base-pixel borders, halo rows) on the structured kernel
 *   DSPH_OPT_FORK           1 (default) / 0: the BFS-tile launch of a large forward on a plan-owned side stream
 *   DSPH_OPT_STRIP_MINROWS  least height of a strip rectangle in tiles, default 4                      (tuning)
 *   DSPH_OPT_STRIP_FORM     which strip kernel takes the rectangles of the 64 -> 64, K = 5, three-term shape: 0 (default) the
 *                           quad strips of round 5 (64-column strips, four pixels per lane, csrc/cheb_qstrip_kernel.h),
 *                           1 the strip pairs of round 3 (32-column strips, csrc/cheb_strip_kernel.h).  Same rectangles, same
 *                           arithmetic, another order of summation inside a row: equal to rounding, not bit for bit.
 *   DSPH_OPT_SPLIT          K > 5: 0 (default) the faster of the two routes by rule, 1 always the product identity
 *                           T_{4+j} = 2 T_4 T_j - T_{|4-j|} (passes of K <= 5 on the fast kernels), 2 never
 *   DSPH_OPT_TSTEP          1 (default) / 0: graphs wider than the fused kernels take (ELL width 13 .. 32: the reference's 20
 *                           neighbours) run every recurrence step through LDS tiles (csrc/cheb_tstep.hip); 0: the gather kernel.
 *                           Same bits either way.
 *   DSPH_OPT_PACK           1 (default) / 0: a layer with at most four input channels and at most 16 output columns (the first
 *                           layers of a network; likewise eight channels and 32 columns, two maps) runs its batch four maps to
 *                           an item on the tile kernels when the batch has more
 *                           than one map (the input-side strips put two maps on a wave whatever the batch: map n always rides
 *                           half n & 1, its bits do not depend on the batch).  A map then equals its single-map result
 *                           to rounding, not bit for bit (another order of exact-zero products, and at K = 4 the fp32-equivalent
 *                           arithmetic in its exact-fp32 form); 0 keeps every map's bits independent of the batch. */
#define DSPH_OPT_STRIPS 1
#define DSPH_OPT_STRUCT 2
#define DSPH_OPT_TABLES 3
#define DSPH_OPT_FORK 4
/* (5 and 7 were DSPH_OPT_STRIP_SEG and DSPH_OPT_STRIP_GENERIC: unknown options now, DSPH_E_BADARG; the numbers are never reused) */
#define DSPH_OPT_STRIP_MINROWS 6
#define DSPH_OPT_SPLIT 8
#define DSPH_OPT_TSTEP 9
#define DSPH_OPT_PACK 10
#define DSPH_OPT_STRIP_FORM 11
/*   DSPH_OPT_F16_XEXP       binary exponent e in [-100, 100], default 0: under DSPH_PREC_F16X3 the quad strips split x 2^e into
 *                           f16 pairs and store y 2^-e (exact both ways); see DSPH_PREC_F16X3 for how to choose it.  Read when a
 *                           forward is enqueued: it may change between forwards (not while one is being enqueued on this plan). */
#define DSPH_OPT_F16_XEXP 12
/*   DSPH_OPT_QSTRIP_IMAGE   0 (default: automatic = on wherever the K = 5 quad strips run) / 1 on / 2 off: the quad-strip forward
 *                           reads the values of L~ from an image packed once per plan and basis -- every strip's rows in the order
 *                           the kernel's LDS ring holds them, moved in by LDS-DMA -- instead of gathering them from the
 *                           direction-ordered copy in every step.  Same bits either way.  The image costs 2,304 bytes per strip
 *                           row (rows ylo - 1 .. yhi + 6 of every strip): about 0.5 GB per basis at nside 1024, next to the
 *                           0.45 GB of the direction-ordered copy that the other kernels keep using; it is built by
 *                           dsph_plan_prepare (Chebyshev basis) or by the first forward of a basis outside a stream capture, and
 *                           freed with the plan's tables and when this option changes.  0: a forward that finds no memory for the
 *                           image, or is being captured before one exists, gathers; 1: no memory is an error (DSPH_E_HIP);
 *                           2: never built (memory-tight callers, and the comparison build).  Does not drop the tables. */
#define DSPH_OPT_QSTRIP_IMAGE 13
int dsph_plan_set_option(dsph_plan* plan, int32_t option, int64_t value);

int64_t dsph_plan_rows(const dsph_plan* plan);
int64_t dsph_plan_cols(const dsph_plan* plan);
int32_t dsph_plan_ell_width(const dsph_plan* plan);
int64_t dsph_plan_out_rows(const dsph_plan* plan, int32_t K); /* rows y is produced for */
/* 1 if the fused kernels can run this (plan, shape) -- in one forward, or, for K > 5 where the plan's options allow it, as the
 * chain of <= 5-term passes; 0 otherwise (the unfused kernels then serve dsph_cheb_forward under DSPH_ALGO_AUTO) */
int dsph_plan_fused_ok(const dsph_plan* plan, int32_t Fin, int32_t Fout, int32_t K);
/* 1 if a forward of this (plan, shape) runs as the chain of <= 5-term passes (K > 5: the product identity, csrc/cheb_split.hip) --
 * every pass of the chain rounds its input to bf16 hi + lo again under DSPH_PREC_BF16X3, so a caller that wants 1e-5 asks for the
 * six-term split there; 0 if one pass of the fused kernels (K <= 10 on the 8-neighbour grid) or the unfused kernels serve it.
 * (Round 6: K = 10 -- the reference tutorials' order -- runs in ONE pass of the breadth-first tile kernel over 9-ring regions
 * where the plan's regions fit its 1,168-row planes, i.e. on the 8-neighbour grid stencil; on wider graphs it stays the chain.) */
int dsph_plan_uses_chain(const dsph_plan* plan, int32_t Fin, int32_t Fout, int32_t K);

/* How the fused forward with K terms splits the plan's 256-row tiles between its two kernels: *n_struct tiles whose
 * (K-1)-ring region was verified to be a square of a 2-D 9-point stencil (structured-tile kernel,
 * csrc/cheb_struct_kernel.h: either the rows of the region are a plain Z-order continuation of the tile's, or the
 * region was laid out from the graph and is addressed through per-tile tables -- base-pixel borders of the sphere, halo
 * rows of a sharded plan) and *n_bfs tiles handled through breadth-first ring tables (csrc/cheb_fused_kernel.h).
 * DSPH_E_UNSUPPORTED when neither kernel can run the plan (the unfused path then serves dsph_cheb_forward). */
int dsph_plan_tile_counts(const dsph_plan* plan, int32_t K, int64_t* n_struct, int64_t* n_bfs);

/* How many of those structured tiles a forward of this shape hands to the strip kernel instead (csrc/cheb_strip_kernel.h:
 * rectangles of at least 3 x 4 tiles whose regions are plain Z-order squares, streamed row by row in 32-column strips with
 * the recurrence in registers -- Clenshaw's backward form, fed by the MFMA).  0 when the strip kernel does not take the shape
 * (it implements K = 5, Fin = Fout = 64 per 64-column block, DSPH_PREC_BF16X3), the plan holds no such rectangle, or the
 * strips would not pay for a batch of N maps (its work items are (pair of strips, map): small or ragged plans need a batch
 * to fill the device; the rule is in csrc/cheb_fused.hip, strips_apply); the other tiles are served as dsph_plan_tile_counts
 * says.  Same summation per output whichever kernel writes it?  No: the two
 * forms round differently (both within the tolerance of their precision), so outputs of tiles that change hands between
 * two plans of the same graph agree to rounding, not bit for bit. */
int dsph_plan_strip_tiles(const dsph_plan* plan, int64_t N, int32_t Fin, int32_t Fout, int32_t K, int32_t precision,
                          int64_t* n_tiles);

/* The strip kernel's work list for K terms, for tests and tools: `out` receives up to `capacity` records of twelve int32 --
 * x0[2], w[2] (first output column and output width of the two strips of the pair), xs[2] (column of lane 0), y0, y1 (output
 * rows [y0, y1)), xlo, xhi, ylo, yhi (the clamp rectangle) -- in the virtual Z-order plane of the row index (x = even bits,
 * y = odd bits of the row number); *n_pairs the number of pairs the plan holds (also when capacity is smaller). */
int dsph_plan_strip_pairs(const dsph_plan* plan, int32_t K, int32_t* out, int64_t capacity, int64_t* n_pairs);
/* (With the quad strips -- DSPH_OPT_STRIP_FORM 0, K = 5 -- a record is ONE 64-column strip, uncut along y: x0[0], w[0], xs[0] and
 * w[1] = 0.  The kernel cuts the rows at run time: the rows of all strips laid end to end form one tape per map, cut into
 * `pieces` equal pieces, `wg_per_piece` workgroups per piece each taking every wg_per_piece-th map of the batch; a strip is cut
 * wherever a piece ends.  This call reports that split for a batch of N maps -- for tests and tools that want to look at the seams.) */
int dsph_plan_strip_split(const dsph_plan* plan, int64_t N, int32_t* grid, int32_t* pieces, int32_t* wg_per_piece, int64_t* tape_rows);
/* (Round 6: the rectangles of the quad strips are found on the LOGICAL tile grid -- tiles on a border between two base pixels, or
 * between two superpixels of a compacted partial-sky map, belong to them wherever the neighbouring tiles continue the pixel grid by
 * a pure translation -- and a strip's record is in the coordinates of its rectangle's plane: the rectangle's first pixel is
 * (16, 16), one ring of tiles around it is addressable.  Which ROW of the map a pixel of that plane is, the strip's table says:
 * this call looks up n pixels xy[2 i], xy[2 i + 1] of record `strip` (clamped to the rectangle and its halo as the kernel clamps
 * them; K = 5: y to [ylo - 1, yhi + 6] -- that kernel reads a row as it comes, a run of steps touches these rows of the ring
 * tiles, past the halo for nothing) into rows[i].  For the strip pairs (DSPH_OPT_STRIP_FORM 1) the plane is the virtual Z-order plane of the row index itself.) */
int dsph_plan_strip_rows(const dsph_plan* plan, int32_t K, int64_t strip, int64_t n, const int32_t* xy, int64_t* rows);
/* The packed image of L~ of K = 5 quad-strip record `strip` (DSPH_OPT_QSTRIP_IMAGE), for tests and tools: yhi - ylo + 8 rows, the
 * rows y = ylo - 1 .. yhi + 6 of the strip's plane, 576 floats each: [v = 0 the diagonal, v = 1 + d direction d (W NW N NE E SE S
 * SW)][p = 0..15][t = 0..3] = that value of L~ of the pixel (clamp(xs + 4 p + t, xlo, xhi), y), times two for
 * basis = DSPH_BASIS_CHEBYSHEV.  *n_floats the strip's floats (also when capacity is smaller; nothing is copied then).  Builds
 * the image of that basis if the plan has none yet; DSPH_E_UNSUPPORTED without quad strips or with the option off. */
int dsph_plan_strip_image(const dsph_plan* plan, int32_t basis, int64_t strip, float* out, int64_t capacity, int64_t* n_floats);

/* Pointer and workspace contract of the Chebyshev family (dsph_cheb_forward / dsph_poly_forward*, dsph_poly_forward_pool,
 * dsph_cheb_planes, dsph_cheb_step, dsph_cheb_contract, dsph_cheb_backward_weights, dsph_cheb_wgrad).  Every device pointer is a
 * contiguous fp32 array, 4-byte aligned at least.  A pointer that a kernel of the call would access in 16-byte pieces is
 * checked on the host first: the call then either takes a kernel that accesses it by the element (same values, to rounding where
 * the other kernel sums in another order) or returns DSPH_E_BADARG before anything is launched, with a message that names the
 * pointer and the requirement.  Per entry point, "any" = any 4-byte alignment:
 *   unfused route (DSPH_ALGO_UNFUSED, or DSPH_ALGO_AUTO on a plan / shape without fused kernels), dsph_cheb_step,
 *   dsph_cheb_contract, dsph_cheb_wgrad: x / in / prev / out / planes[k] / w / bias / y / dy / dw any (16-byte accesses where the
 *       channel count is a multiple of four and the pointer aligned, chosen per launch; a y off alignment with Fout % 4 == 0 is
 *       contracted by the exact-fp32 kernels instead of the MFMA one); the workspace any.
 *   fused route (DSPH_ALGO_FUSED, or DSPH_ALGO_AUTO where dsph_plan_fused_ok, the chain of passes of K > 5 included):
 *       x      16-byte aligned when Fin % 4 == 0 (refused otherwise: DSPH_ALGO_AUTO resolves the route from plan and shape alone,
 *              as dsph_workspace_bytes must, and does not fall back); any when Fin % 4 != 0 (the kernels read a padded copy)
 *       w      any (read by the element into the packed weight images)
 *       bias   any; off 16-byte alignment the tiles of the quad-strip kernels (K = 5, 64 -> 64 j; K = 8, 32 -> 32) run on the tile kernels
 *       y      any; off 16-byte alignment the tiles of every strip kernel run on the tile kernels, which then store by the element
 *       y_pooled, y_scratch (dsph_poly_forward_pool)  16-byte aligned (refused otherwise; y_scratch may be NULL)
 *       planes (dsph_cheb_planes)  16-byte aligned, as x; DSPH_ALGO_AUTO runs the dsph_cheb_step kernels when x or planes is not
 *              (no workspace depends on the choice), DSPH_ALGO_FUSED refuses
 *       dy     any; off 16-byte alignment the quad-strip weight gradient's pixels go to the tile kernel (same workspace)
 *       dw     any
 *       workspace  16-byte aligned (refused otherwise), at least the bytes of the size query: weight images, the padded copy of x,
 *              the buffers of the chain of passes, the slabs of the weight gradient all lie inside them.
 * No call writes to x, w, bias or dy, or outside y / y_pooled / planes / dw and the queried bytes of the workspace
 * (tests/test_gpu_cheb_memory.py holds every route to this with guard bands and checksums). */

/* Bytes of scratch dsph_cheb_forward needs for this call shape (0 is possible).  It has no pointers to look at: the route it sizes
 * is a function of plan, shape and algo alone, and the forward keeps to that route. */
size_t dsph_workspace_bytes(const dsph_plan* plan, int64_t N, int32_t Fin, int32_t Fout,
                            int32_t K, int32_t precision, int32_t algo);

/* The whole forward:  y[n,m,o] = act( sum_f sum_k (T_k(L~) x[n,:,f])[m] * w[f*K + k, o] + bias[o] )
 * Replaces: Chebyshev.call (gnn_layers.py:131-150, 155-159) including the K-1 calls of
 * utils.split_sparse_dense_matmul (utils.py:49-78) and tf.matmul (gnn_layers.py:149).
 *   x     device (N, n_cols, Fin) fp32, channels fastest, NEST pixel order as given by the caller
 *   w     device [Fin*K, Fout] fp32, row index f*K + k  (the reference's `kernel` variable)
 *   bias  device [Fout] fp32 or NULL                    (the reference's `bias`, shape [1,1,Fout])
 *   y     device (N, out_rows, Fout) fp32
 * Batch normalisation (gnn_layers.py:152-153) sits between the contraction and the bias in the
 * reference.  With the moving statistics (inference; center=False, scale=False) it is a per-channel scale and shift,
 * s[o] = 1 / sqrt(var[o] + eps): the caller passes w[:, o] * s[o] as `w` and bias[o] - mean[o] * s[o] as `bias` and gets
 * act(BN(conv) + bias) from this one call (deepsphere/gnn_layers.py does, keyed on the versions of the statistics); with
 * batch statistics (training) a layer calls this with bias=NULL, act=NONE and finishes with dsph_bn_stats and dsph_bn_apply.
 * Asynchronous on `hip_stream` (a hipStream_t; NULL = the default stream).  (Part of a large fused forward may run on a
 * stream the plan owns, forked from and joined back into `hip_stream` inside the call: invisible to the caller, capturable.)
 * Alignment (the family's contract above): on the fused route x (Fin % 4 == 0) and the workspace must be 16-byte aligned --
 * DSPH_E_BADARG "x must be 16-byte aligned" otherwise, also under DSPH_ALGO_AUTO --, w, bias and y may sit at any 4-byte
 * alignment (a misaligned y or bias moves tiles from the strip kernels to the tile kernels); the unfused route takes any pointer. */
int dsph_cheb_forward(const dsph_plan* plan, const float* x, const float* w, const float* bias,
                      float* y, int64_t N, int32_t Fin, int32_t Fout, int32_t K, int32_t act,
                      int32_t precision, int32_t algo, void* workspace, size_t workspace_bytes,
                      void* hip_stream);

/* The same forward for either polynomial basis (dsph_cheb_forward is this with
 * DSPH_BASIS_CHEBYSHEV).  With DSPH_BASIS_MONOMIAL it replaces Monomial.call
 * (gnn_layers.py:262-309): same layouts, same weight row order f*K + k. */
int dsph_poly_forward(const dsph_plan* plan, const float* x, const float* w, const float* bias,
                      float* y, int64_t N, int32_t Fin, int32_t Fout, int32_t K, int32_t basis,
                      int32_t act, int32_t precision, int32_t algo, void* workspace,
                      size_t workspace_bytes, void* hip_stream);

/* The same forward restricted to a subset of the output tiles (fused kernel only; DSPH_E_UNSUPPORTED otherwise):
 * DSPH_PART_INTERIOR = the 256-row tiles whose whole (K-1)-hop region lies inside the plan's output rows, i.e. on
 * a sharded plan the tiles that read no halo row of another rank; DSPH_PART_BOUNDARY = the others.  Launching
 * INTERIOR while the halo exchange is in flight and BOUNDARY after it hides the exchange behind the interior
 * (deepsphere/sharding.py).  INTERIOR + BOUNDARY write exactly the rows DSPH_PART_ALL writes, with the same bits.
 * Each part finalises exactly the rows of its own tiles (with an activation other than NONE / RELU: the kernels write the
 * pre-activation and one elementwise pass over those tiles' rows follows inside the same call), so the two parts may be
 * issued in either order, alone, or repeated. */
#define DSPH_PART_ALL 0
#define DSPH_PART_INTERIOR 1
#define DSPH_PART_BOUNDARY 2
int dsph_poly_forward_part(const dsph_plan* plan, const float* x, const float* w, const float* bias,
                           float* y, int64_t N, int32_t Fin, int32_t Fout, int32_t K, int32_t basis,
                           int32_t act, int32_t precision, int32_t algo, int32_t part, void* workspace,
                           size_t workspace_bytes, void* hip_stream);

/* The same with flags:
 *   DSPH_FWD_KEEP_WEIGHTS  `workspace` still holds the weight images that the previous call on this workspace packed from the
 *                          same w (values, not only pointer), Fin, Fout, K, basis, precision and batch class (N == 1 or N > 1:
 *                          layers with at most four input channels and 16 output columns pack four maps into one item of the
 *                          tile kernels when there is more than one, with a block-diagonal image): the fused kernels use them as
 *                          they are and the call launches no weight-preparation kernel (three small launches per forward
 *                          otherwise; on a small map they are a third of the forward).  The caller vouches for it -- a layer
 *                          in inference does, by the version counter of its kernel tensor (deepsphere/gnn_layers.py).  The
 *                          unfused path packs nothing and ignores the flag. */
#define DSPH_FWD_KEEP_WEIGHTS 1
int dsph_poly_forward_ex(const dsph_plan* plan, const float* x, const float* w, const float* bias,
                         float* y, int64_t N, int32_t Fin, int32_t Fout, int32_t K, int32_t basis,
                         int32_t act, int32_t precision, int32_t algo, int32_t part, int32_t flags, void* workspace,
                         size_t workspace_bytes, void* hip_stream);

/* The forward followed by HealpyPool(p = 1) (reference healpy_layers.py:20-63: MaxPool1D / AveragePooling1D with pool size 4 over
 * the NEST-ordered pixels, after gnn_layers.py:106-161) in one call: y_pooled (N, n_rows / 4, Fout) = pool(act(conv(x) + bias)).
 * The input-side strip kernels and both tile kernels reduce the four children in their store step and write the pooled map
 * only -- the full-resolution output of a 1 -> 16 layer is 16 times its input and, with the pooling's read of it, most of that
 * layer's time; `y_scratch` is not used any more (every kernel pools in
 * its store) and may be NULL.  Same values as the two calls (bit for bit for the maximum; the mean adds the
 * children in the same order).  pool_type: DSPH_POOL_MAX | DSPH_POOL_AVG.  Availability: dsph_plan_pool_fusable (whole
 * unsharded maps of whole tiles, a width that is a multiple of four, activation none or ReLU, not the 64 -> 64 shape where the
 * Clenshaw strip kernel takes tiles); DSPH_E_UNSUPPORTED otherwise -- run
 * dsph_poly_forward and dsph_healpix_pool then.  Workspace and flags as dsph_poly_forward_ex.
 * Alignment: x (Fin % 4 == 0), y_pooled, y_scratch (unless NULL) and the workspace 16-byte aligned -- every kernel stores the pooled
 * map in 16-byte pieces; DSPH_E_BADARG naming the pointer otherwise --, w and bias any 4-byte alignment. */
int dsph_plan_pool_fusable(const dsph_plan* plan, int64_t N, int32_t Fin, int32_t Fout, int32_t K, int32_t act);
int dsph_poly_forward_pool(const dsph_plan* plan, const float* x, const float* w, const float* bias, float* y_scratch,
                           float* y_pooled, int64_t N, int32_t Fin, int32_t Fout, int32_t K, int32_t basis, int32_t act,
                           int32_t precision, int32_t pool_type, int32_t flags, void* workspace, size_t workspace_bytes,
                           void* hip_stream);

/* One recurrence step on (N, n_cols, F) planes:  out = alpha * (L~ @ in) - beta * prev
 * for rows [0, rows) of every map (rows <= n_rows; rows <= 0 means n_rows); prev may be NULL
 * when beta == 0.  Replaces one utils.split_sparse_dense_matmul call plus the `2*... - x0`
 * temporaries (gnn_layers.py:138,141).  Exposed for the one-ring-halo-per-step sharded mode,
 * where the host exchanges boundary rows between steps, and for tests.
 * Alignment: in, prev and out at any 4-byte alignment; float4 accesses when F % 4 == 0 and all three are 16-byte aligned, else
 * the kernels' scalar form (the same additions in the same order: the same bits). */
int dsph_cheb_step(const dsph_plan* plan, const float* in, const float* prev, float* out,
                   int64_t N, int32_t F, float alpha, float beta, int64_t rows, void* hip_stream);
/* Note on plans with halo columns (n_cols > n_rows): a step writes rows [0, rows) only, so a SECOND step would
 * gather halo entries nobody produced.  The multi-step entry points (dsph_cheb_forward / dsph_poly_forward*,
 * dsph_cheb_planes, dsph_cheb_backward_weights) therefore return DSPH_E_BADARG for K > 2 on such a plan unless a
 * shrinking schedule was installed with dsph_plan_set_levels; drive dsph_cheb_step yourself, exchanging the halo
 * between steps, for the one-ring-per-step mode. */

/* The dense contraction alone on K planes of shape (N, plane_rows, Fin), plane k at
 * planes[k] (device pointers in a HOST array of K entries):
 *   y[n,m,o] = act( sum_k sum_f planes[k][n,m,f] * w[f*K + k, o] + bias[o] ),  m < rows.
 * Replaces tf.stack/reshape/transpose/matmul (gnn_layers.py:144-150).
 * Where the plain contraction kernel runs (the batch is a grid dimension there) N is at most 65535: DSPH_E_UNSUPPORTED beyond,
 * reported after the device has been selected.
 * Alignment: every plane, w, bias and y at any 4-byte alignment.  Planes are loaded in 16-byte pieces only when Fin % 4 == 0 and
 * all K are aligned; a y off alignment with Fout % 4 == 0 is written by the exact-fp32 kernels (by the element) instead of the
 * MFMA kernel, whatever `precision` asks for. */
int dsph_cheb_contract(const float* const* planes, int64_t plane_rows, const float* w,
                       const float* bias, float* y, int64_t N, int64_t rows, int32_t Fin,
                       int32_t Fout, int32_t K, int32_t act, int32_t precision, int device,
                       void* hip_stream);

/* The planes T_1 x .. T_{K-1} x alone (T_0 x = x), without the contraction: `planes` receives K-1
 * arrays of x's shape (N, n_cols, Fin) back to back, valid on the plan's output rows.  This is the left
 * operand of the weight gradient, rebuilt in the backward pass: the same recurrence as
 * gnn_layers.py:134-143, run by the fused tile kernel (no MFMA, the tile rows of every plane are
 * stored from LDS) when the plan/shape allows, else by K-1 dsph_cheb_step launches.
 * `algo`: DSPH_ALGO_AUTO | UNFUSED | FUSED as in dsph_cheb_forward.
 * Alignment: the fused kernel loads x and stores the planes in 16-byte pieces.  DSPH_ALGO_AUTO runs the step kernels instead when
 * x or planes is off 16-byte alignment (this call has no workspace whose size would depend on it); DSPH_ALGO_FUSED returns
 * DSPH_E_BADARG naming x or planes; DSPH_ALGO_UNFUSED takes any 4-byte alignment. */
int dsph_cheb_planes(const dsph_plan* plan, const float* x, float* planes, int64_t N, int32_t Fin,
                     int32_t K, int32_t basis, int32_t algo, void* hip_stream);

/* Weight gradient of the layer (training):
 *     dw[f*K + k, o] = sum_{n, m < out_rows} (T_k(L~) x)[n,m,f] * dy[n,m,o]
 * from the layer input x (N, n_cols, Fin) and the upstream gradient dy (N, out_rows, Fout).  The reference
 * has no counterpart of its own: TensorFlow differentiates the op sequence of gnn_layers.py:131-150.
 * When the fused tile kernel applies (dsph_plan_fused_ok) the planes never leave the LDS: each tile's T_k
 * is contracted over its pixels against dy -- `precision` DSPH_PREC_FP32: exact-fp32 MFMAs; DSPH_PREC_BF16X3: both
 * operands split hi + lo, three bf16 MFMAs per product term, fp32 accumulate (fused path only) -- and the
 * per-workgroup partial sums are reduced in a fixed order (deterministic).  Otherwise: dsph_cheb_planes into `workspace`, then
 * dsph_cheb_wgrad.  `algo` as in dsph_cheb_forward.
 * K = 5, Fin = 64, Fout a multiple of 64, DSPH_PREC_BF16X3, on a whole-graph plan whose forward of that shape runs on the quad
 * strips and whose matrix equals its transpose (checked entry for entry, to fp32 rounding): the strips' pixels go through the
 * quad-strip weight-gradient kernel (csrc/cheb_qwgrad_kernel.h: the recurrence to order two on x AND on dy, orders 3 and 4 from
 * the product rule of the polynomials), the other tiles through the tile kernel; same result to the arithmetic's rounding
 * (measured 4 - 7e-6 of max |dw| against float64), 2.2 x faster at BASELINE configs[2].  A non-symmetric matrix, another shape
 * or DSPH_PREC_FP32 keep every tile on the tile kernel.
 * In the bf16 arithmetic every second workgroup of both kernels contracts against -dy and its partial sum is subtracted: the
 * matrix pipe's fp32 accumulation of long sums is biased towards minus infinity (1 - 2e-5 of max |dw| at configs[2]) and the
 * mirror cancels it.
 * Alignment: on the fused route the workspace and x (Fin % 4 == 0; otherwise a padded copy behind the slabs is read) must be 16-byte
 * aligned: DSPH_E_BADARG naming the pointer, before any launch.  dy at any 4-byte alignment: the quad-strip kernel reads it in
 * 16-byte pieces, so a dy off alignment sends every tile to the tile kernel (the workspace holds its slabs either way).  dw any.
 * The unfused route takes any pointer.  The workspace query's bytes cover the slabs of both kernels, the padded copy of x, or the
 * planes and dsph_cheb_wgrad's slabs. */
size_t dsph_backward_weights_workspace_bytes(const dsph_plan* plan, int64_t N, int32_t Fin, int32_t Fout,
                                             int32_t K, int32_t algo);
int dsph_cheb_backward_weights(const dsph_plan* plan, const float* x, const float* dy, float* dw, int64_t N,
                               int32_t Fin, int32_t Fout, int32_t K, int32_t basis, int32_t precision, int32_t algo,
                               void* workspace, size_t workspace_bytes, void* hip_stream);

/* Weight gradient (training):  dw[f*K + k, o] = sum_{n, m < rows} planes[k][n,m,f] * dy[n,m,o]
 * for K planes T_k x of shape (N, plane_rows, Fin) (HOST array of K device pointers, e.g. x and the
 * outputs of dsph_cheb_step) and an upstream gradient dy (N, rows, Fout).  The reference has no
 * counterpart of its own: TensorFlow differentiates tf.matmul (gnn_layers.py:149).  Deterministic
 * (fixed-order reduction of per-workgroup partial sums held in `workspace`).
 * Alignment: planes, dy, dw and the workspace at any 4-byte alignment (read and written by the element). */
size_t dsph_wgrad_workspace_bytes(int64_t N, int64_t rows, int32_t Fin, int32_t Fout, int32_t K);
int dsph_cheb_wgrad(const float* const* planes, int64_t plane_rows, const float* dy, float* dw,
                    int64_t N, int64_t rows, int32_t Fin, int32_t Fout, int32_t K, void* workspace,
                    size_t workspace_bytes, int device, void* hip_stream);

/* Gather / scatter of boundary rows for the halo exchange of the sharded path:
 *   pack:   buf[n, i, :] = src[n, idx[i], :]       src (N, src_rows, F), buf (N, n_idx, F)
 *   unpack: dst[n, idx[i], :] = buf[n, i, :]
 * idx is a DEVICE int32 array. */
int dsph_rows_pack(const float* src, int64_t src_rows, const int32_t* idx, int64_t n_idx,
                   float* buf, int64_t N, int32_t F, int device, void* hip_stream);
int dsph_rows_unpack(float* dst, int64_t dst_rows, const int32_t* idx, int64_t n_idx,
                     const float* buf, int64_t N, int32_t F, int device, void* hip_stream);

/* Skip connection of a residual block (reference gnn_layers.GCNN_ResidualLayer.call, gnn_layers.py:407-413: tf.add and
 * the activation, three elementwise ops over the whole map) in ONE pass, in place over n contiguous floats:
 *   act_before == 0:  y = act(y + alpha * skip)          act_before != 0:  y = act(y) + alpha * skip
 * act is a DSPH_ACT_* code (DSPH_ACT_NONE with alpha = 1 is the reference's activation=None case, x + input). */
int dsph_residual_epilogue(float* y, const float* skip, int64_t n, float alpha, int32_t act, int32_t act_before,
                           int device, void* hip_stream);

/* Pooling over the 4^p NEST children of a HEALPix pixel, the step between two convolutions of every reference model.
 * Replaces: the Keras MaxPool1D / AveragePooling1D inside healpy_layers.HealpyPool.call (healpy_layers.py:48-63,77-85;
 * pool_size = strides = 4^p, padding "valid", channels last).
 *   x  device (N, rows_out * group, F) fp32      y  device (N, rows_out, F) fp32      group = 4^p
 *   y[n, m, f] = max | mean over i < group of x[n, group * m + i, f]
 * The backward (the reference gets it from TensorFlow's autodiff): dx[n, group * m + i, f] = dy[n, m, f] / group for the mean;
 * for the maximum dy[n, m, f] at the first child that holds it and 0 at the others (x: the forward input; may be NULL for the mean).
 * group at most 2^20 (DSPH_E_UNSUPPORTED beyond, before any HIP call); every offset is 64-bit, the grid is capped at 2^20
 * workgroups and walked grid-stride. */
#define DSPH_POOL_MAX 0
#define DSPH_POOL_AVG 1
int dsph_healpix_pool(const float* x, float* y, int64_t N, int64_t rows_out, int32_t F, int32_t group, int32_t type, int device,
                      void* hip_stream);
int dsph_healpix_pool_backward(const float* x, const float* dy, float* dx, int64_t N, int64_t rows_out, int32_t F, int32_t group,
                               int32_t type, int device, void* hip_stream);

/* RING <-> NEST reordering of full-sky HEALPix maps (plan-free; csrc/healpix_reorder.hip).
 * Replaces: hp.reorder(m, r2n=True) in front of healpy_networks.HealpyGCNN and hp.reorder(m, n2r=True) behind it (the reference's
 * workflow for maps stored in RING order, healpy's default), i.e. a gather through an int64 table of 12 nside^2 entries.
 *   x, y     device (N, 12 nside^2, F) fp32, contiguous; they must not overlap
 *   to_nest  1: x is in RING order, y in NEST order;  0: x is in NEST order, y in RING order
 *     y[n, nest(p), f] = x[n, p, f]  (to_nest = 1),   y[n, p, f] = x[n, nest(p), f]  (to_nest = 0),   p a RING index
 * No table: a workgroup owns an aligned block of pixels of one face (one run of NEST rows) and computes every pixel's RING index
 * from (face, ix, iy); rows under 32 floats turn through an LDS image of the block, wider rows are copied row by row.  Values are
 * moved, never computed: bit for bit.  Vector accesses where F is a multiple of 4 (2) and the maps are aligned, scalar otherwise.
 * nside a power of two, 1 <= nside <= 8192 (pixel indices are int32; DSPH_E_UNSUPPORTED beyond), F >= 1, N >= 0 (N = 0: DSPH_OK,
 * no launch); every element offset is 64-bit.  Grid: the blocks of one map x min(N, 65535); further maps on further trips.
 * Bad arguments (NULL, nside not a power of two, F < 1, N < 0, to_nest not 0 or 1, x overlapping y): DSPH_E_BADARG before any launch.
 * Only enqueues on `hip_stream`. */
int dsph_healpix_reorder(const float* x, float* y, int64_t N, int32_t nside, int32_t F, int32_t to_nest, int device, void* hip_stream);

/* The k nearest pixels of every pixel of a (partial) HEALPix map in NEST order (plan-free; csrc/healpix_knn.hip).
 * Replaces: the k-d tree over all pixel centres behind the graphs of HealpyGCNN (reference healpy_networks.py:110-118 asks the
 * pygsp fork for SphereHealpix(k = n_neighbors); healpix.healpix_graph(mode="knn") here), for graphs built on the device.
 *   indices  device int64 [M], sorted NEST ids of the set; NULL: the full sky, M = 12 nside^2 and row = NEST id
 *   lut      device int32 [12 nside^2], NEST id -> row of the set or -1; NULL exactly when indices is
 *   nbr      device int32 [M, k]   rows of the k nearest other pixels of the set, ascending by (d2, row)
 *   d2       device float64 [M, k] their squared chord distances between pixel centres (the geometry of healpix.pix2vec)
 *   ok       device uint8 [M]      1: the row is guaranteed; 0: the search window held fewer than k pixels of the set, or the k-th
 *                                  distance found is not below the radius the window provably covers -- the row's contents are then
 *                                  unspecified and the caller completes it.  On the full sky every row comes out 1 for k <= 60.
 * One wave per pixel, candidates from a window of rings and ring positions held in registers, k rounds of a wave-wide arg-min;
 * float64 throughout; no workspace, no atomics, one writer per element.
 * nside a power of two, 1 <= nside <= 8192 (pixel indices are int32; DSPH_E_UNSUPPORTED beyond), 1 <= k <= 64 (DSPH_E_UNSUPPORTED
 * beyond), k < M <= 12 nside^2.  Bad arguments (a required pointer NULL, indices without lut or lut without indices, nside not a
 * power of two, k < 1, M <= k, M != 12 nside^2 without indices): DSPH_E_BADARG before any launch.  Only enqueues on `hip_stream`. */
int dsph_healpix_knn(int32_t nside, int32_t k, const int64_t* indices, const int32_t* lut, int64_t M, int32_t* nbr, double* d2,
                     uint8_t* ok, int device, void* hip_stream);

/* The kernel matrix of HealpySmoothing built on the device (plan-free; csrc/healpix_disc.hip).
 * Replaces: the BallTree / k-d tree over all pixel centres, its two queries per pixel and the numpy sort and normalisation behind
 * HealpySmoothing (reference healpy_layers.py:640-720; HealpySmoothing._build_tree and _finish_table here).
 * `indices`, `lut` and M as for dsph_healpix_knn (the ids need not be sorted: row i is the pixel indices[i]).
 *
 * dsph_healpix_disc_count: for every pixel of the set, how many pixels of the set lie within the squared chord r2 of it (<=, the
 * pixel itself included).  r2 = (2 sin(rho / 2))^2 for a disc of radius rho <= pi, 0 <= r2 <= 4.
 *   count    device int32 [M]
 *   ok       device uint8 [M]   1: the count is guaranteed (every guard of the window lies beyond r2); 0: the caller counts that row
 *
 * dsph_healpix_gauss_table: for every pixel one finished row of the matrix: the W nearest pixels of the set, the pixel itself
 * included, selected by (squared chord, row) ascending.
 *   W          entries per row, 1 <= W <= 512 (DSPH_E_UNSUPPORTED beyond), W <= M
 *   sigma_rad  standard deviation of the Gaussian in radians
 *   rho        the radius the window must cover, 0 < rho <= pi (the kernel's window reaches 1.125 rho); a window of more than 2048
 *              candidates: DSPH_E_UNSUPPORTED
 *   cols     device int32 [M, W]    the columns of the row, ascending
 *   vals     device float32 [M, W]  with theta = 2 asin(min(chord / 2, 1)): exp(-0.5 / sigma^2 * theta^2) in float64, rounded to
 *                                   float32, divided by the float64 sum of the row's float32 values, rounded to float32
 *   raw      device float32 [M, W]  the values before the division (the reference's cache files hold these); may be NULL
 *   ok       device uint8 [M]       1: W pixels were found and the W-th squared chord lies below the smallest guard; 0: the row
 *                                   is the caller's to complete (cols = -1 where fewer than W pixels were found)
 * A pixel id outside [0, 12 nside^2): ok = 0, cols = -1, nothing read.  One workgroup per row, candidates and selection in LDS,
 * float64 distances; no workspace, no global atomics, one writer per element; element offsets are 64-bit (M W may pass 2^31).
 * nside a power of two, 1 <= nside <= 8192 (DSPH_E_UNSUPPORTED beyond).  Bad arguments (a required pointer NULL, indices without
 * lut or the reverse, nside not a power of two, M < 1, M != 12 nside^2 without indices, W < 1, W > M, sigma_rad <= 0, rho or r2 out
 * of range): DSPH_E_BADARG before any launch.  Both only enqueue on `hip_stream`. */
int dsph_healpix_disc_count(int32_t nside, double r2, const int64_t* indices, const int32_t* lut, int64_t M, int32_t* count,
                            uint8_t* ok, int device, void* hip_stream);
int dsph_healpix_gauss_table(int32_t nside, int32_t W, double sigma_rad, double rho, const int64_t* indices, const int32_t* lut,
                             int64_t M, int32_t* cols, float* vals, float* raw, uint8_t* ok, int device, void* hip_stream);

/* Rotating scalar HEALPix maps in NEST order by bilinear interpolation (plan-free; csrc/healpix_interp.hip).
 * Replaces: hp.Rotator.rotate_map_pixel on the host (random-rotation augmentation of a training loop), or a 4-entry-per-row sparse
 * table per rotation (32 bytes per pixel and rotation).
 * `indices`, `lut` and M as for dsph_healpix_knn; NULL, NULL and M = 12 nside^2: the full sky.
 *
 * dsph_healpix_rotate:  y[n, r, :] = sum_j w_j x[n, row(p_j), :], where (p_j, w_j), j < 4, is the interpolation stencil of healpy's
 * get_interp_weights at the direction R^T v(indices[r]), v the pixel centre and R = rot[n] (rot[0] when n_rot == 1).
 *   x, y     device (N, M, F) fp32, contiguous; they must not overlap
 *   rot      device float64 [n_rot, 9], row-major 3 x 3 rotation matrices; n_rot == 1 (one for the batch) or n_rot == N
 * A source pixel outside the set contributes zero and the other weights are not renormalised: the result is the rotated zero-padded
 * full-sky map read at the set.  An id of `indices` outside [0, 12 nside^2) gives a row of zeros.
 * Geometry in float64 (centre, rotation, atan2, ring above, weights); weights rounded to float32 once; w0 x0 and three fused
 * multiply-adds in float32 in the order of the stencil: deterministic, no atomics, one writer per element.  The stencil of a pixel
 * is computed once per (sample, pixel) -- once per pixel with n_rot == 1 -- and reused over the F channels.  F < 16: a lane per
 * pixel; wider rows: stencils through LDS and lanes along the channels; 1, 2 or 4 floats per access by F and the alignment of x, y.
 * Grid: blocks of 256 rows x min(N, 65535); further maps on further trips.  Every element offset is 64-bit.
 *
 * dsph_healpix_interp_table: the same stencils for ONE rotation as a table, cols int32 [M, 4] (rows of x) and vals float32 [M, 4];
 * a source outside the set becomes (col = the row itself, val = 0), the padding of dsph_ell_smooth.  dsph_ell_smooth on it applies
 * the rotation, on its transpose (entries regrouped by column) the adjoint.  No row holds a column twice but for that padding.
 *
 * nside a power of two, 1 <= nside <= 8192 (pixel indices are int32; DSPH_E_UNSUPPORTED beyond), F >= 1, N >= 0 (N = 0 or M = 0:
 * DSPH_OK, no launch).  Bad arguments (a required pointer NULL, indices without lut or the reverse, nside not a power of two,
 * M != 12 nside^2 without indices, M outside [0, 12 nside^2], F < 1, N < 0, n_rot neither 1 nor N, rot not 8-byte aligned, x
 * overlapping y): DSPH_E_BADARG before any launch.  Both only enqueue on `hip_stream`. */
int dsph_healpix_rotate(const float* x, float* y, int64_t N, int32_t nside, int32_t F, const double* rot, int64_t n_rot,
                        const int32_t* lut, const int64_t* indices, int64_t M, int device, void* hip_stream);
int dsph_healpix_interp_table(int32_t nside, const double* rot, const int32_t* lut, const int64_t* indices, int64_t M, int32_t* cols,
                              float* vals, int device, void* hip_stream);

/* Spherical harmonic transforms of scalar HEALPix maps in NEST order (plan-free; csrc/healpix_sht.hip).
 * Replaces: hp.map2alm / hp.alm2map / hp.anafast on the host (copy, reorder to RING, seconds per map at nside 1024, no gradient).
 * Equal pixel weights w = 4 pi / (12 nside^2) (healpy with use_weights=False), no iteration: healpy's `iter` is a composition of
 * the two transforms and belongs to the caller.  Two stages each way, each an entry point of its own:
 *   dsph_sht_ring_analysis       fm[m, ring, c]  = sum_j x[ring, j, c] e^{-i m phi_j}
 *   dsph_sht_legendre_analysis   alm[n, (l, m), f] = w sum_ring lambda_lm(theta_ring) fm[m, ring, c]
 *   dsph_sht_legendre_synthesis  fm[m, ring, c]  = sum_{l >= m} alm[n, (l, m), f] lambda_lm(theta_ring)
 *   dsph_sht_ring_synthesis      y[ring, j, c]   = Re sum_m c_m fm[m, ring, c] e^{+i m phi_j},  c_0 = 1, c_m = 2 (m > 0)
 * with c = n F + f the C = N F columns (map x channel), ring = 1 .. 4 nside - 1 from the north pole, lambda_lm the normalised
 * associated Legendre functions (Y_lm = lambda_lm e^{i m phi}), mmax = lmax.
 *   x, y   device (N, M, F) fp32, contiguous, any 4-byte alignment (read and written a float at a time)
 *   fm     device float64 [mmax + 1][4 nside - 1][C][2], (re, im) pairs: 16 (mmax + 1)(4 nside - 1) bytes per column, 200 MB at
 *          nside 1024 and mmax 3071 -- the caller's scratch, and the caller's to chunk over the maps
 *   alm    device float64 [N][nalm][F][2], healpy's packed layout: index m (2 lmax + 1 - m) / 2 + l, nalm = (lmax + 1)(lmax + 2) / 2
 *          (a torch complex128 tensor (N, nalm, F))
 *   lut, indices, M   the footprint as for dsph_healpix_rotate; NULL, NULL and M = 12 nside^2: the full sky.  Analysis counts a
 *          pixel outside the footprint as zero; synthesis writes the footprint's rows and nothing else.  `indices` itself is not
 *          read (the rings are walked through lut)
 * float64 throughout: the ring phase m phi_j is reduced exactly in integers (m (2 j - 1 - kshift) mod 8 nr) before the sine and
 * cosine, every 16th term; the terms between by a rotation with the equally reduced step.  A direct DFT: m above a ring's Nyquist
 * needs no folding.  The Legendre recurrence in l carries an integer scale beside its value (steps of 2^480), so that
 * lambda_mm = O(sin^m theta) may start hundreds of orders below float64's range; a term on a negative scale (below 2^-240 of a
 * function of order 1) is dropped.  lambda_lm(pi - theta) = (-1)^(l + m) lambda_lm(theta) halves the recurrences.  Deterministic:
 * no atomics, one writer per element, the sums over rings and over l in a fixed order.  Grids: (ring, blocks of m or of pixels,
 * min(blocks of 8 columns, 4096)) and (m, min(blocks of 8 columns, 4096)); further columns on further trips; 64-bit offsets.
 *
 * nside a power of two, 1 <= nside <= 2048 (DSPH_E_UNSUPPORTED beyond), 0 <= lmax = mmax <= 4 nside - 1, F >= 1, N >= 0 (N = 0:
 * DSPH_OK, no launch).  Bad arguments (a required pointer NULL, fm or alm not 8-byte aligned, indices without lut or the reverse,
 * M != 12 nside^2 without indices, M outside [0, 12 nside^2], nside not a power of two, lmax out of range, F < 1, N < 0, input
 * overlapping output): DSPH_E_BADARG before any launch.  All four only enqueue on `hip_stream`. */
int dsph_sht_ring_analysis(const float* x, double* fm, int64_t N, int32_t nside, int32_t F, int32_t mmax, const int32_t* lut,
                           const int64_t* indices, int64_t M, int device, void* hip_stream);
int dsph_sht_legendre_analysis(const double* fm, double* alm, int64_t N, int32_t nside, int32_t F, int32_t lmax, int device,
                               void* hip_stream);
int dsph_sht_legendre_synthesis(const double* alm, double* fm, int64_t N, int32_t nside, int32_t F, int32_t lmax, int device,
                                void* hip_stream);
int dsph_sht_ring_synthesis(const double* fm, float* y, int64_t N, int32_t nside, int32_t F, int32_t mmax, const int32_t* lut,
                            const int64_t* indices, int64_t M, int device, void* hip_stream);

/* Attention over the edges of the pixel graph (plan-free; csrc/nbr_attention.hip).
 * Replaces: gnn_transformers.scaled_dot_product_sparse_attention (reference gnn_transformers.py:54-106: three embedding lookups that
 * materialise q, k, v per edge, exp, two segment sums) and the split_heads transposes around it (:189-196, :225-231).
 *   q, k, v  device (N, M, heads * depth) fp32, channels last, rows `ld` floats apart (ld >= heads * depth: three views of one
 *            (N, M, 3 heads depth) projection need no copy); head h is channels [h depth, (h + 1) depth)
 *   nbr      device int32 [M][width]: the neighbours of row i first, -1 in the unused slots; summed in slot order; an entry
 *            outside [0, M) counts as unused
 *   out      device (N, M, heads * depth), contiguous:  out[n,i,h] = sum_j softmax_j(q_i,h . k_j,h / sqrt(depth)) v_j,h
 *   lse      device (N, M, heads) or NULL:  log sum_j exp(q_i,h . k_j,h / sqrt(depth)), what the backward needs
 * The softmax is the stable form (running maximum); the reference exponentiates the raw logits, which is the same number until
 * it overflows (logits above 88).  A row without neighbours gives out = 0 and lse = 0 (the reference: 0 / 0).
 * Shapes: depth one of 4, 8, 16, 32, 64; heads >= 1 with heads * depth <= 256; width >= 1; ld a multiple of 4; q, k, v, out
 * 16-byte aligned; M at most 2^31 - 1 (the table's row indices are int32; N * M * d may pass 2^31: every offset is 64-bit).
 * Anything else: DSPH_E_BADARG with the limit named in the message, before any HIP call; there is no slower path.
 *
 * The backward (the reference: TensorFlow's autodiff), from the forward's out and lse and the upstream gradient dout (contiguous,
 * out's shape): dq, dk, dv with rows ld_grad floats apart.  nbrT [M][widthT] is the table of the transposed graph (row j lists
 * the i whose row names j; pass nbr again for a symmetric graph).  `delta` is scratch of N * M * heads floats (the call writes
 * delta[n,i,h] = dout_i,h . out_i,h there).  No atomics: every element has one writer and a fixed order of summation, so two
 * runs agree bit for bit.  Two launches.  Both calls only enqueue on `hip_stream`. */
int dsph_nbr_attention_forward(const float* q, const float* k, const float* v, int64_t ld, float* out, float* lse,
                               const int32_t* nbr, int32_t width, int64_t N, int64_t M, int32_t heads, int32_t depth, int device,
                               void* hip_stream);
int dsph_nbr_attention_backward(const float* q, const float* k, const float* v, int64_t ld, const float* out, const float* lse,
                                const float* dout, const int32_t* nbr, int32_t width, const int32_t* nbrT, int32_t widthT,
                                float* delta, float* dq, float* dk, float* dv, int64_t ld_grad, int64_t N, int64_t M, int32_t heads,
                                int32_t depth, int device, void* hip_stream);

/* Dense attention: every row attends to every row of its map (plan-free; csrc/dense_attention.hip, kernels in
 * csrc/dense_attention_kernel.h).
 * Replaces: gnn_transformers.scaled_dot_product_attention (reference gnn_transformers.py:14-51: matmul, softmax over a materialised
 * (N, heads, M, M) tensor of logits, matmul) with mask = None -- what Graph_ViT (:248-356) and Healpy_ViT (healpy_layers.py:381-414)
 * run on -- and the split_heads transposes around it (:189-196, :225-231).
 *   q, k, v  device (N, M, heads * depth) fp32, channels last, rows `ld` floats apart (ld >= heads * depth: three views of one
 *            (N, M, 3 heads depth) projection need no copy); head h is channels [h depth, (h + 1) depth)
 *   out      device (N, M, heads * depth), contiguous:  out[n,i,h] = sum_j softmax_j(q_i,h . k_j,h / sqrt(depth)) v_j,h, j over [0, M)
 *   lse      device (N, M, heads) or NULL:  log sum_j exp(q_i,h . k_j,h / sqrt(depth)), what the backward needs
 * Flash style: key tiles stream through LDS, the softmax is the online, stable form, all products are exact-fp32 MFMA; no logit is
 * written to global memory and nothing of size M^2 is allocated.
 * Shapes: depth one of 4, 8, 16, 32, 64; heads >= 1 with heads * depth <= 256; M >= 1 (any value: tails are masked); ld a multiple
 * of 4; q, k, v, out 16-byte aligned.  Anything else: DSPH_E_BADARG with the limit named in the message, before any device call;
 * there is no slower path.
 *
 * The backward (the reference: TensorFlow's autodiff), from the forward's out and lse and the upstream gradient dout (contiguous,
 * out's shape): dq, dk, dv with rows ld_grad floats apart.  `delta` is scratch of N * M * heads floats (the call writes
 * delta[n,i,h] = dout_i,h . out_i,h there); the library allocates nothing.  No atomics: every element has one writer and a fixed
 * order of summation, so two runs agree bit for bit.  Two launches (query blocks: delta and dq; key blocks: dk and dv; the
 * probabilities are recomputed from lse).  Both calls only enqueue on `hip_stream`. */
int dsph_dense_attention_forward(const float* q, const float* k, const float* v, int64_t ld, float* out, float* lse, int64_t N,
                                 int64_t M, int32_t heads, int32_t depth, int device, void* hip_stream);
int dsph_dense_attention_backward(const float* q, const float* k, const float* v, int64_t ld, const float* out, const float* lse,
                                  const float* dout, float* delta, float* dq, float* dk, float* dv, int64_t ld_grad, int64_t N,
                                  int64_t M, int32_t heads, int32_t depth, int device, void* hip_stream);

/* The same two calls with a choice of arithmetic for their matrix products (the same kernels over the arithmetic policy of
 * csrc/dense_attention_split.hip); everything above holds, argument checks and messages included.  `precision`:
 *   DSPH_PREC_FP32    the two entry points above, bit for bit (every depth)
 *   DSPH_PREC_BF16X6  every product (q k^T, p v, dout v^T, ds k, ds^T q, p^T dout) on v_mfma_f32_16x16x32_bf16 with both operands
 *                     split into three bf16 terms, six partial products, fp32 accumulation: fp32-equivalent
 *   DSPH_PREC_BF16X3  two terms, three partial products: operands carry 16 significant bits
 * Each term is the round-to-nearest bf16 of the running remainder; bf16 has fp32's exponent range, so there is no scale rule and
 * no range condition.  The softmax statistics, exp, lse, delta and the rescalings stay fp32.  Same blocking, layouts, tails and
 * determinism (one writer per element, no atomics) as the fp32 kernels.
 * The split arithmetics run depth 32 and 64 (the contraction fills the instruction's K = 32); at depth 4, 8 or 16 they return
 * DSPH_E_UNSUPPORTED naming the depths 32, 64, before any launch -- there is no fallback to fp32.  Any other precision code
 * (DSPH_PREC_F16X3 included): DSPH_E_BADARG. */
int dsph_dense_attention_forward_prec(const float* q, const float* k, const float* v, int64_t ld, float* out, float* lse, int64_t N,
                                      int64_t M, int32_t heads, int32_t depth, int32_t precision, int device, void* hip_stream);
int dsph_dense_attention_backward_prec(const float* q, const float* k, const float* v, int64_t ld, const float* out, const float* lse,
                                       const float* dout, float* delta, float* dq, float* dk, float* dv, int64_t ld_grad, int64_t N,
                                       int64_t M, int32_t heads, int32_t depth, int32_t precision, int device, void* hip_stream);

/* The same two calls with the reference's `mask` argument (gnn_transformers.py:14-51: `logits += mask * -1e9` before the softmax):
 *   x_ij = s_ij + mask_ij * (-1e9),   s_ij = q_i . k_j / sqrt(depth) in fp32 after the scale,
 * the product mask * -1e9f rounded to fp32, then added in fp32 -- in all three arithmetics on the fp32 logit, after the product;
 * the mask is never split.  It is an ADD, not a select: 1 is "do not attend", 0 "attend", a fraction a soft bias (2.5e-9 lowers a
 * logit by 2.5).  A row whose keys are all masked behaves as in the reference: fp32 has an ulp of 64 at 1e9, so -1e9 + s is exactly
 * -1e9 for |s| < 32, the row's softmax is uniform and its output the mean of v; nothing is NaN.
 *   mask     device fp32; element (n, h, i, j) -- map, head, query row, key -- is
 *            mask[n * mask_stride_batch + h * mask_stride_head + i * mask_stride_query + j].  The key stride is 1; each of the
 *            three strides may be 0 (broadcast), none negative.  So one operand is a shared key mask (M,) [0, 0, 0], a per-map
 *            key mask (N, 1, 1, M) [M, 0, 0], a per-head one [0, M, 0], a shared pair mask (M, M) [0, 0, M] or a full
 *            (N, heads, M, M) one.  Rows need no alignment (16-byte loads where the address allows, single loads elsewhere).
 *            Never read at a key index >= M nor for a query row >= M: the last row may end where the allocation ends.
 *   stat     device (N, M, heads, 2), 8-byte aligned (forward: or NULL): the row statistic as the PAIR (m, log l), m = max_j x_ij,
 *            l = sum_j exp(x_ij - m).  Not their sum: on a fully masked row m = -1e9 and m + log l rounds back to m, from which
 *            the backward would recompute p = 1 instead of 1 / M.  The backward takes p = exp((x - m) - log l).
 * Everything else -- layouts, shapes, precisions (a split at a depth other than 32, 64: DSPH_E_UNSUPPORTED), tails (keys past M
 * stay at -inf), determinism (two backward launches, no atomics, one writer per element), messages naming the limit -- is as in
 * the _prec calls, whose arguments these take besides.  A NULL mask or a negative stride: DSPH_E_BADARG.  The unmasked calls
 * above run the code they ran before; a mask of zeros gives their `out` bit for bit. */
int dsph_dense_attention_forward_masked(const float* q, const float* k, const float* v, int64_t ld, float* out, float* stat,
                                        const float* mask, int64_t mask_stride_batch, int64_t mask_stride_head,
                                        int64_t mask_stride_query, int64_t N, int64_t M, int32_t heads, int32_t depth,
                                        int32_t precision, int device, void* hip_stream);
int dsph_dense_attention_backward_masked(const float* q, const float* k, const float* v, int64_t ld, const float* out,
                                         const float* stat, const float* mask, int64_t mask_stride_batch, int64_t mask_stride_head,
                                         int64_t mask_stride_query, const float* dout, float* delta, float* dq, float* dk, float* dv,
                                         int64_t ld_grad, int64_t N, int64_t M, int32_t heads, int32_t depth, int32_t precision,
                                         int device, void* hip_stream);

/* One pass of Gaussian smoothing: a wide-row ELL matrix over a map of few channels (plan-free; csrc/ell_smooth.hip).
 * Replaces: one utils.split_sparse_dense_matmul per channel and repetition of healpy_layers.HealpySmoothing.call (reference
 * healpy_layers.py:725-764) with the transposes, the unstack / stack and the mask multiply around them.
 *   cols, vals  device int32 / fp32 [M][W], row-major: row m of the kernel matrix, every row W entries.  An entry outside [0, M)
 *               counts as an empty slot.  The transposed table, padded with col = row, val = 0, gives the input gradient.
 *   x, y        device (N, M, C) fp32, contiguous, the caller's layout; they must not overlap (a pass cannot run in place)
 *   reps        device int32 [C] or NULL: channel c is smoothed if reps == NULL or reps[c] > pass, copied through otherwise
 *   mask        device fp32 [M][mask_C] or NULL, mask_C = 1 or C: the stored value (smoothed or copied) is multiplied by
 *               mask[m * mask_C + (mask_C == 1 ? 0 : c)]
 *     y[n,m,c] = sum_j vals[m,j] * x[n, cols[m,j], c]
 * A group of 16 (W <= 128) or 64 lanes owns a row and keeps its entries in registers over the batch and channel loops, so the table
 * is read from memory once per call; sums are a fused multiply-add chain per lane and a fixed butterfly: no atomics, one writer,
 * bitwise reproducible.  Any W >= 1 and C >= 1 (C = 1, 2 and multiples of 4 with 16-byte aligned maps take vector loads).
 * M at most 2^31 - 1 (the table's columns are int32; N * M * C may pass 2^31: every offset is 64-bit).
 * Bad arguments (NULL, M > 2^31 - 1, W <= 0, C <= 0, pass < 0, mask_C not 1 or C, x overlapping y): DSPH_E_BADARG before any launch.
 * Only enqueues on `hip_stream`. */
int dsph_ell_smooth(const int32_t* cols, const float* vals, int64_t M, int32_t W, const float* x, float* y, int64_t N, int32_t C,
                    const int32_t* reps, int32_t pass, const float* mask, int32_t mask_C, int device, void* hip_stream);

/* A change of polynomial basis on a layer's weights (plan-free; csrc/basis_change.hip): what makes gnn_layers.Bernstein a
 * Chebyshev layer.  With row i of `coeff` the Chebyshev coefficients of the layer's i-th polynomial B_i,
 *     sum_i B_i(L~) x W_i = sum_j T_j(L~) x W'_j,   W'_j = sum_i coeff[i][j] W_i,
 * so the layer runs dsph_poly_forward / dsph_cheb_backward_weights with Kp terms on W' (transpose = 0), and the weight gradient
 * those return goes back through the transposed map (transpose = 1).  Replaces the K (K + 1) sparse products per call of the
 * reference's Bernstein.call (gnn_layers.py:543-554).
 *   w, w_out  device fp32 [Fin * Kp, Fout], row index f * Kp + i, contiguous; they must not overlap
 *   coeff     device fp32 [Kp, Kp], row-major, 1 <= Kp <= 64
 *     w_out[f*Kp + j, o] = sum_i c(i,j) * w[f*Kp + i, o]
 *       c(i,j) = coeff[i*Kp + j]   (transpose = 0: weights into the kernels' basis)
 *       c(i,j) = coeff[j*Kp + i]   (transpose = 1: the weight gradient back out)
 * Each output is one fp32 fma chain over i = 0 .. Kp - 1 in that order, one writer per element: bitwise reproducible.  Vector
 * loads and stores of 4 (2) floats where Fout is a multiple of 4 (2) and the pointers are aligned, scalar ones otherwise.
 * Bad arguments (NULL, Kp outside [1, 64], Fin or Fout < 1, transpose not 0 or 1, w_out overlapping w or coeff): DSPH_E_BADARG
 * before any launch.  One launch; only enqueues on `hip_stream` (no allocation, no synchronisation, no copy: legal under
 * stream capture). */
int dsph_basis_change(const float* w, const float* coeff, float* w_out, int32_t Fin, int32_t Fout, int32_t Kp, int32_t transpose,
                      int device, void* hip_stream);

/* Batch normalisation with batch statistics over a channels-last map (plan-free; csrc/batch_norm.hip), the epilogue fused:
 *     z[r, c] = act((y[r, c] - mean[c]) * rstd[c] * gamma[c] + shift[c]),   y, z device (rows, F) fp32, contiguous, rows = N * M
 * Replaces, in a training step: the Keras BatchNormalization between the contraction and the bias (reference gnn_layers.py:152-159)
 * and inside GCNN_ResidualLayer.call (:395-405) with the bias add and the activation behind it, and their gradients from
 * TensorFlow's autodiff.  Three passes over the map forward (statistics: one read; apply: one read, one write), seven backward.
 * Any F >= 1 (there is no cap on F; 16-byte accesses where F % 4 == 0 and the maps are 16-byte aligned, 8-byte ones for even F
 * and 8-byte alignment, else scalar); rows up to 2^40 and rows * F up to 2^62 (DSPH_E_UNSUPPORTED beyond); every offset is 64-bit.
 * Bad arguments (a required pointer NULL, rows < 1, F < 1, an unknown activation, eps <= 0, momentum outside [0, 1], rows = 1
 * together with running_var): DSPH_E_BADARG with the entry point named in the message, before any HIP call.  Every call only
 * enqueues on `hip_stream`: no allocation, no synchronisation, no atomics -- legal under stream capture, and two calls on the
 * same input give the same bits.
 *
 * Workspace of the two reducing calls, caller-owned, 8-byte aligned, a function of the shape alone:
 *     P = max(1, min(2048, rows, ceil(rows * F / 8192)))  partial results per channel,   bytes = 16 * F * (P + 1)
 * (P workgroups each reduce a contiguous range of rows to one partial per channel; one workgroup per channel merges the P
 * partials in a fixed order in float64.)
 *
 * Statistics: mean[c], var[c] (biased: sum (y - mean)^2 / rows) and rstd[c] = 1 / sqrt(var[c] + eps), device [F] each, all three
 * required.  Partial (count, mean, M2) triples merged by Chan's formula in float64, never E[y^2] - E[y]^2: a channel whose mean is
 * large against its spread keeps its digits.  mean_lo, rstd_lo: device [F] or NULL -- what the fp32 mean and rstd rounded away
 * (mean = mean[c] + mean_lo[c] to 2^-48), for dsph_bn_backward.  running_mean / running_var: device [F] or NULL; when given they are updated on the
 * device as torch.nn.BatchNorm1d does, running = (1 - momentum) * running + momentum * batch, the variance with the UNBIASED
 * batch variance var * rows / (rows - 1) (Keras uses the biased one).  Two launches. */
size_t dsph_bn_workspace_bytes(int64_t rows, int32_t F);
int dsph_bn_stats(const float* y, int64_t rows, int32_t F, float eps, float* mean, float* var, float* rstd, float* mean_lo, float* rstd_lo,
                  float* running_mean, float* running_var, float momentum, void* workspace, size_t workspace_bytes, int device, void* hip_stream);
/* The elementwise pass alone.  mean, rstd: device [F], plain arrays -- the batch statistics of the call above, or the moving mean
 * and 1 / sqrt(running_var + eps) for the inference form.  gamma, shift: device [F] or NULL (1 and 0).  act: a DSPH_ACT_* code.
 * z may be y (in place); any other overlap of the two is not allowed.  One launch. */
int dsph_bn_apply(const float* y, float* z, int64_t rows, int32_t F, const float* mean, const float* rstd, const float* gamma,
                  const float* shift, int32_t act, int device, void* hip_stream);
/* The backward of the two calls together, from the forward's input y, its output z and the upstream gradient dz (rows, F):
 *     g = dz * act'(z)      (from the OUTPUT: relu z > 0, elu z > 0 ? 1 : z + 1, sigmoid z (1 - z), tanh 1 - z^2; with DSPH_ACT_NONE z
 *                            is not read and may be NULL)
 *     x^ = (y - mean) * rstd                                  (recomputed)
 *     dshift[c] = s1 = sum_r g,   dgamma[c] = s2 = sum_r g x^   (device [F] or NULL: not wanted)
 *     dy = gamma * rstd * (g - s1 / rows - x^ * s2 / rows)      (device (rows, F); must not overlap y, z or dz)
 * mean_lo, rstd_lo: device [F] or NULL (0): the low parts from dsph_bn_stats.  x^, the sums and dy are evaluated in float64 on mean +
 * mean_lo and rstd + rstd_lo: with few rows dy is a cancellation (two rows, eps = 1e-5: down to 4e-5 of g) that one fp32 rounding of
 * either array would swamp; without the low parts the result is only as good as the fp32 arrays.
 * gamma: device [F] or NULL (1).  Three launches: the reduction of s1 and s2 by the scheme of the statistics (partials, then the
 * fixed-order merge), then one elementwise pass.  Workspace as above. */
int dsph_bn_backward(const float* y, const float* z, const float* dz, const float* mean, const float* rstd, const float* mean_lo,
                     const float* rstd_lo, const float* gamma, float* dy,
                     float* dgamma, float* dshift, int64_t rows, int32_t F, int32_t act, void* workspace, size_t workspace_bytes, int device,
                     void* hip_stream);

/* Layer normalisation over the trailing axis of a channels-last map (plan-free; csrc/layer_norm.hip), the residual add in front of
 * it fused:
 *     a[r, :] = x[r, :] + res[r, :]   (written to sum; res and sum both NULL: a = x)
 *     z[r, c] = (a[r, c] - mean[r]) * rstd[r] * gamma[c] + beta[c],   mean, var (biased) over the d channels of row r,
 *                                                                      rstd = 1 / sqrt(var + eps)
 * x, res, sum, z device (rows, d) fp32, contiguous, rows = N * M; gamma, beta device [d] or NULL (1 and 0).  Replaces the Keras
 * LayerNormalization(axis=-1) of GCNN_ResidualLayer (reference gnn_layers.py:373-374) and the two of a transformer block with
 * the add between them (gnn_transformers.py:149-245), and their gradients from TensorFlow's autodiff.
 * 1 <= d <= 1024 (a row lives in the registers of 1 .. 64 lanes; 16-byte accesses where d % 4 == 0 and every map of the call is
 * 16-byte aligned, scalar ones otherwise); rows up to 2^40 (DSPH_E_UNSUPPORTED beyond); every offset is 64-bit; rows == 0 succeeds
 * without a launch.  The row's mean, its centred sum of squares (never E[a^2] - E[a]^2), rstd and x^ are float64.
 * Bad arguments (a required pointer NULL, res without sum or sum without res, rows < 0, d outside [1, 1024], eps <= 0, a written
 * map overlapping another map of the call, a workspace that is NULL or misaligned): DSPH_E_BADARG with the entry point named in
 * the message; a workspace that is too small: DSPH_E_WORKSPACE; both before any HIP call.  The one overlap allowed is sum == x or
 * sum == res (in place, the same pointer).  Every call only enqueues on `hip_stream`: no allocation, no synchronisation, no
 * atomics -- legal under stream capture, and two calls on the same input give the same bits.  A row that holds a NaN or Inf gives
 * a non-finite row of z and da (and non-finite dgamma, dbeta) and leaves every other row as it would be without it.
 * The forward is ONE launch: every input is read once, every output written once. */
int dsph_ln_forward(const float* x, const float* res, float* sum, float* z, int64_t rows, int32_t d, float eps, const float* gamma,
                    const float* beta, int device, void* hip_stream);
/* The backward, from the forward's normalised input a (sum, or x when there was no res), the upstream gradient dz of z and the
 * gradient dsum that reached the sum output (NULL: none):
 *     x^ = (a - mean) * rstd   (mean and rstd recomputed from a in float64: nothing is saved between the two calls)
 *     g = dz * gamma,   da = rstd * (g - mean_d(g) - x^ * mean_d(g x^)) + dsum      (the gradient of x and of res alike)
 *     dbeta[c] = sum_r dz,   dgamma[c] = sum_r dz x^                                 (device [d] or NULL: not wanted)
 * da: device (rows, d), overlapping none of a, dz, dsum (those three are only read and may coincide).  Two launches: the row
 * pass, whose P = max(1, min(2048, ceil(rows / 4), ceil(rows * d / 8192))) workgroups each leave one float64 partial per channel
 * in the workspace, and the merge of the P partials in a fixed order (skipped, and no workspace needed, when neither dgamma nor
 * dbeta is wanted).  Workspace: caller-owned, 8-byte aligned, dsph_ln_workspace_bytes(rows, d) = 16 * d * P bytes, a function of
 * the shape alone (0 for a shape the entry points do not take, and for rows == 0). */
size_t dsph_ln_workspace_bytes(int64_t rows, int32_t d);
int dsph_ln_backward(const float* a, const float* dz, const float* dsum, const float* gamma, float eps, float* da, float* dgamma,
                     float* dbeta, int64_t rows, int32_t d, void* workspace, size_t workspace_bytes, int device, void* hip_stream);

/* The pseudo-convolutions as one row GEMM with the bias and the activation in its store (plan-free; csrc/patch_gemm.hip):
 *     Y[r, c] = act( sum_j X[r, j] * W[j, c] + bias[c mod P] )
 * x device (R, Kd) fp32, rows contiguous; w device (Kd, C); y device (R, C); bias device [P] or NULL (none); act a DSPH_ACT_* code.
 * HealpyPseudoConv (reference healpy_layers.py:81-146, Conv1D with kernel = stride = g = 4^p on a NEST map (N, M, Fin)):
 *     R = N M / g, Kd = g Fin, C = P = Fout, W[i Fin + f, o] = weight[o, f, i];
 * HealpyPseudoConv_Transpose (:149-216): R = N M, Kd = Fin, C = g Fout, P = Fout, W[f, i Fout + o] = weight[f, o, i].
 * Both x views are free reshapes of the map.  ONE launch: every row of x is read once per group of up to 128 output columns,
 * y is written once.  precision: DSPH_PREC_FP32 (v_mfma_f32_32x32x2_f32), DSPH_PREC_BF16X6 or DSPH_PREC_BF16X3, fp32
 * accumulation in all three; DSPH_PREC_F16X3 has no scale rule here and runs DSPH_PREC_BF16X6.
 * Any R in [1, 2^40], Kd and C in [1, 4096] (DSPH_E_UNSUPPORTED beyond); Kd or C not a multiple of four, or x / y off 16-byte
 * alignment: scalar accesses of the same elements.  Bad arguments (x, w or y NULL; R, Kd, C or P < 1; C % P != 0; an unknown act
 * or precision; y overlapping x or w): DSPH_E_BADARG with the entry point named in the message, before any HIP call.  The call
 * only enqueues on `hip_stream`: no allocation, no synchronisation, no copy -- legal under stream capture. */
int dsph_patch_gemm(const float* x, const float* w, const float* bias, float* y, int64_t R, int32_t Kd, int32_t C, int32_t P, int32_t act,
                    int32_t precision, int device, void* hip_stream);
/* The gradient of that epilogue, from the stored output y and the upstream gradient dy (both device (R, C)):
 *     dZ = dY * act'(Y)   (relu y > 0, elu y > 0 ? 1 : y + 1, sigmoid y (1 - y), tanh 1 - y^2; DSPH_ACT_NONE: dZ = dY, y may be NULL)
 *     dbias[o] = sum_r sum_{c = o mod P} dZ[r, c]            (device [P], or NULL: not wanted)
 * dz may be dy itself (in place) and overlaps nothing else.  The P' = max(1, min(2048, ceil(R C / 8192))) workgroups of the
 * map pass each leave one float64 partial per bias element in the workspace and a second launch merges them in a fixed order: no
 * atomics, the same call twice gives the same bits.  Workspace: caller-owned, 8-byte aligned,
 * dsph_patch_backward_workspace_bytes(R, C, P) = 8 P P' bytes, a function of the shape alone (0 for a shape the entry point does
 * not take); not needed (may be NULL) when dbias is NULL.  Errors as dsph_patch_gemm; a workspace that is too small:
 * DSPH_E_WORKSPACE.  The rest of the layer's backward reuses what exists: dX = dZ W^T is dsph_patch_gemm on the transposed weight
 * image without bias and activation, dW = X^T dZ is dsph_cheb_wgrad on the one plane X viewed as (1, R, Kd). */
size_t dsph_patch_backward_workspace_bytes(int64_t R, int32_t C, int32_t P);
int dsph_patch_epilogue_backward(const float* y, const float* dy, float* dz, float* dbias, int64_t R, int32_t C, int32_t P, int32_t act,
                                 void* workspace, size_t workspace_bytes, int device, void* hip_stream);

const char* dsph_last_error(void);
int dsph_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DSPHERE_H */
