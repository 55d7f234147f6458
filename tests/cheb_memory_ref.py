"""Case table and float64 references of the Chebyshev family's memory-contract tests (tests/test_gpu_cheb_memory.py; not
collected by pytest).  One entry per route of DESIGN.md's alignment audit, at the smallest shape that still reaches the kernel;
``data(case)`` builds the graph, the inputs and ONE map-sized oracle result per case on the host and caches them, so that the
pointer variants of a case (x, y, w, bias, dy, dw pushed off 16-byte alignment) share it.  tests/test_cheb_memory_host.py checks on
the CPU that every reference is finite and has the sizes the table says.

Graphs are built on the host alone (the host test has no GPU): the full-sphere 8-neighbour grid Laplacian in the ELL layout of
``healpix.grid_laplacian_ell`` -- the matrix ``bench.build_laplacian`` / ``_grid_ell`` rescale with a Lanczos estimate made on the
device -- rescaled with lmax = 2, the bound of a normalised Laplacian's spectrum; the k-NN graphs as ``test_tiled_step_on_wide_graphs``
builds them; the sphere without its last pixels as ``test_quad_strips_on_a_map_with_an_incomplete_last_tile`` cuts it.

Tolerances (max|got - ref| / max|ref|, ``helpers.rel_err``) are the ones the existing test of the same route and arithmetic
uses: 2e-6 for fp32 / bf16x6 / f16x3, 1e-5 for bf16x3 at Fin >= 16 and 2e-5 below, five times that behind tanh, 2e-5 of max|dW|
for weight gradients."""

import functools
from collections import namedtuple

import numpy as np
from scipy import sparse

from oracle import cheb_oracle as orc

# kind: forward | pool | planes | wgrad | parts;  graph: (builder, *args);  opts: plan options by the names of deepsphere._native
# algo / prec / basis / act: by name;  route: what the GPU test asserts through plan.tile_counts / plan.strip_tiles before it runs:
#   unfused   the plan has no fused kernels for the shape, or ALGO_UNFUSED is asked for
#   bfs       every tile on the BFS-tile kernel, no structured tile
#   struct    structured tiles, none of them on a strip kernel
#   strips    strip_tiles > 0 (the strip kernel is the one opts and shape select)
#   chain     the chain of <= 5-term passes (plan.uses_chain)
# y_off: what a y off 16-byte alignment does, by the audit: "same" -- the same kernels with scalar stores, bit-equal to the aligned
#   run; "tiles" -- the strips' tiles go to the tile kernels: bit-equal to a STRIPS_NEVER plan's aligned run, within twice the
#   tolerance of this plan's; "close" -- another kernel takes over (the unfused contraction's fall-back, the strips of the chain's last
#   pass): within twice the tolerance.
# bias_off: the same three words for a bias off alignment (only the quad-strip kernels load bias in 16-byte pieces).
Case = namedtuple("Case", "name kind graph N Fin Fout K basis act bias prec algo opts route y_off bias_off")


def _c(name, kind, graph, N, Fin, Fout, K, prec, route, basis="chebyshev", act=None, bias=False, algo="auto", opts=(), y_off="same",
       bias_off="same"):
    return Case(name, kind, graph, N, Fin, Fout, K, basis, act, bias, prec, algo, tuple(opts), route, y_off, bias_off)


ALWAYS = (("OPT_STRIPS", "STRIPS_ALWAYS"),)
NEVER = (("OPT_STRIPS", "STRIPS_NEVER"),)
PAIRS = ALWAYS + (("OPT_STRIP_FORM", "STRIP_FORM_PAIRS"),)

CASES = [
    # ---- unfused step + contract (cheb_step.hip, cheb_tcontract.hip; y off with Fout % 4 == 0: cheb_contract.hip's kernels)
    _c("unfused_8_12_4", "forward", ("knn", 8, 8), 2, 8, 12, 4, "bf16x3", "unfused", act="relu", bias=True, algo="unfused", y_off="close"),
    _c("unfused_7_70_3", "forward", ("knn", 8, 8), 2, 7, 70, 3, "fp32", "unfused", bias=True, algo="unfused"),
    # ---- tiled step / tiled contract on a wide graph (cheb_tstep.hip): the smallest graph of test_tiled_step_on_wide_graphs
    _c("tiled_wide_4_12_3", "forward", ("knn", 16, 20), 2, 4, 12, 3, "bf16x6", "unfused", basis="monomial", act="relu", bias=True, y_off="close"),
    # ---- BFS-tile kernel (cheb_fused_kernel.h), and four maps per item
    _c("bfs_16_32_5", "forward", ("knn", 16, 8), 2, 16, 32, 5, "bf16x3", "bfs", act="relu", bias=True, algo="fused"),
    _c("bfs_16_32_5_fp32", "forward", ("knn", 16, 8), 2, 16, 32, 5, "fp32", "bfs", act="tanh", bias=True, algo="fused"),
    _c("bfs_pack_4_16_5", "forward", ("knn", 16, 8), 4, 4, 16, 5, "bf16x6", "bfs", bias=True, algo="fused"),
    # ---- structured-tile kernel (cheb_struct_kernel.h)
    _c("struct_16_32_5", "forward", ("grid", 32), 2, 16, 32, 5, "bf16x3", "struct", act="relu", bias=True, algo="fused", opts=NEVER),
    # ---- strip pairs (cheb_strip_kernel.h)
    _c("pairs_64_64_5", "forward", ("grid", 128), 1, 64, 64, 5, "bf16x3", "strips", basis="monomial", act="relu", bias=True, algo="fused",
       opts=PAIRS, y_off="tiles"),
    # ---- quad strips, packed image of L~ on (cheb_qstrip_kernel.h); the second one's second column block is w + 64, y + 64
    _c("quad_64_64_5", "forward", ("grid", 64), 3, 64, 64, 5, "bf16x3", "strips", act="relu", bias=True, algo="fused", opts=ALWAYS,
       y_off="tiles", bias_off="tiles"),
    _c("quad_64_128_5", "forward", ("grid", 64), 1, 64, 128, 5, "bf16x3", "strips", bias=True, algo="fused", opts=ALWAYS, y_off="tiles",
       bias_off="tiles"),
    # ---- quad strips beside an incomplete last tile
    _c("quad_drop293", "forward", ("grid_drop", 128, 293), 2, 64, 64, 5, "bf16x3", "strips", act="relu", bias=True, algo="fused", opts=ALWAYS,
       y_off="tiles", bias_off="tiles"),
    # ---- K = 8 quad strips (cheb_qstrip8_kernel.h)
    _c("q8_32_32_8", "forward", ("grid", 128), 1, 32, 32, 8, "bf16x3", "strips", act="relu", bias=True, algo="fused", opts=ALWAYS, y_off="tiles",
       bias_off="tiles"),
    # ---- input-side strips (cheb_istrip_kernel.h); elu: the deferred activation pass
    _c("istrip_16_32_5", "forward", ("grid", 128), 2, 16, 32, 5, "bf16x3", "strips", act="relu", bias=True, algo="fused", opts=ALWAYS, y_off="tiles"),
    _c("istrip_12_40_3", "forward", ("grid", 128), 2, 12, 40, 3, "bf16x6", "strips", act="elu", bias=True, algo="fused", opts=ALWAYS, y_off="tiles"),
    # ---- level-packed strips: one and two channels (x is read through the padded copy in the workspace)
    _c("lstrip_1_16_5", "forward", ("grid", 128), 4, 1, 16, 5, "bf16x6", "strips", act="relu", bias=True, algo="fused", opts=ALWAYS, y_off="tiles"),
    _c("lstrip_2_40_3", "forward", ("grid", 128), 2, 2, 40, 3, "bf16x6", "strips", bias=True, algo="fused", opts=ALWAYS, y_off="tiles"),
    # ---- high-order split (cheb_split.hip): the K = 6 shape of test_high_order_through_the_product_identity
    _c("chain_8_24_6", "forward", ("grid", 64), 2, 8, 24, 6, "bf16x6", "chain", act="relu", bias=True, opts=(("OPT_SPLIT", "SPLIT_ALWAYS"),),
       y_off="close"),
    # ---- conv + pool: the packed-maps shape of test_conv_and_pool_in_one_forward
    _c("pool_4_8_5", "pool", ("grid", 32), 3, 4, 8, 5, "fp32", "struct", basis="monomial", bias=True),
    # ---- planes, fused (BFS-tile kernel, planes mode) and unfused
    _c("planes_grid_64_5", "planes", ("grid", 16), 2, 64, 0, 5, "fp32", "bfs"),
    _c("planes_knn_16_4", "planes", ("knn", 16, 8), 2, 16, 0, 4, "fp32", "bfs"),
    # ---- weight gradient on the BFS-tile kernel; the second one reads a padded copy of x behind the slabs
    _c("wgrad_bfs_16_24_3", "wgrad", ("grid", 16), 3, 16, 24, 3, "fp32", "bfs", algo="fused"),
    _c("wgrad_bfs_1_16_5", "wgrad", ("grid", 16), 2, 1, 16, 5, "fp32", "bfs", algo="fused"),
    # ---- weight gradient on the quad strips (cheb_qwgrad_kernel.h)
    _c("wgrad_quad_64_64_5", "wgrad", ("grid", 64), 2, 64, 64, 5, "bf16x3", "strips", algo="fused", opts=ALWAYS),
    # ---- weight gradient, unfused (steps + cheb_wgrad.hip): 70 columns = two 32-blocks and six, 7 channels = a quarter block; the GPU
    #      test also runs dsph_cheb_wgrad alone on M - 7 rows, an odd count that ends inside the kernel's trip of eight row pairs
    _c("wgrad_unfused_7_70_3", "wgrad", ("knn", 8, 8), 2, 7, 70, 3, "fp32", "unfused", algo="unfused"),
    # ---- interior + boundary parts of a sharded plan (rank 0 of 2: test_parts_finish_only_their_own_rows)
    _c("parts_16_32_5", "parts", ("shard", 64, 5, 0, 2), 2, 16, 32, 5, "bf16x3", "struct", act="elu", bias=True, algo="fused"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def tolerance(case):
    """The tolerance of the existing test of the same route and arithmetic (see the module's docstring)."""
    if case.kind == "wgrad":
        return 2e-5
    tol = 2e-6 if case.prec in ("fp32", "bf16x6", "f16x3") else (1e-5 if case.Fin >= 16 else 2e-5)
    return 5 * tol if case.act == "tanh" else tol


# ---- graphs ------------------------------------------------------------------------------------------------------------------

def _csr(cols, vals, n_cols=None):
    M, W = cols.shape
    return sparse.csr_matrix((vals.reshape(-1).astype(np.float64), cols.reshape(-1), np.arange(0, W * M + 1, W)), shape=(M, n_cols or M))


@functools.lru_cache(maxsize=None)
def graph(spec):
    """-> dict(cols, vals: the plan's ELL arrays; Lt: the same matrix as float64 CSR; n_cols; out_rows; levels; for a shard also
    whole_Lt (the whole sphere's matrix), local_ids (the global rows of the local columns) and own (the rank's row range))."""
    from deepsphere import healpix, utils

    kind = spec[0]
    if kind == "knn":
        L = healpix.healpix_laplacian(spec[1], n_neighbors=spec[2], mode="knn")
        Lt, _ = orc.prepare_L(L)
        cols, vals = utils.csr_to_ell(Lt)
    elif kind in ("grid", "grid_drop", "shard"):
        cols, vals = healpix.grid_laplacian_ell(spec[1])
        vals = utils.rescale_ell(cols, vals, lmax=2.0, scale=0.75)
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        if kind == "grid_drop":  # the sphere without its last pixels: their columns become empty slots
            M = cols.shape[0] - spec[2]
            cols, vals = cols[:M].copy(), vals[:M].copy()
            gone = cols >= M
            vals[gone] = 0.0
            cols[gone] = np.broadcast_to(np.arange(M, dtype=cols.dtype)[:, None], cols.shape)[gone]
    else:
        raise ValueError(spec)
    g = {"cols": cols, "vals": np.ascontiguousarray(vals, dtype=np.float32), "n_cols": cols.shape[0], "levels": None, "out_rows": cols.shape[0]}
    g["Lt"] = _csr(g["cols"], g["vals"])
    if kind == "shard":
        from deepsphere import sharding

        lay = sharding.ShardLayout(g["cols"], g["vals"], spec[2], spec[3], spec[4])
        g.update(whole_Lt=g["Lt"], cols=lay.local_cols, vals=np.ascontiguousarray(lay.local_vals, dtype=np.float32), n_cols=lay.n_cols,
                 levels=lay.levels, local_ids=lay.local_ids, own=lay.own, out_rows=lay.n_own)
        g["Lt"] = None
    return g


# ---- inputs and the one reference per case ------------------------------------------------------------------------------------

def _act64(v, act):
    if act is None:
        return v
    if act == "relu":
        return np.maximum(v, 0.0)
    if act == "elu":
        return np.where(v > 0, v, np.expm1(np.minimum(v, 0.0)))
    if act == "tanh":
        return np.tanh(v)
    raise ValueError(act)


def _forward64(Lt, x, w, K, basis, bias, act, rows):
    """act(sum_k T_k(Lt) x W_k + bias) in float64 on the first ``rows`` rows."""
    planes = orc.chebyshev_planes(Lt, x, K) if basis == "chebyshev" else orc.monomial_planes(Lt, x, K)
    N, M, Fin = x.shape
    # one GEMM: the kernel's rows are f * K + k
    y = (np.ascontiguousarray(planes[:, :, :rows].transpose(1, 2, 3, 0)).reshape(N * rows, Fin * K) @ w.astype(np.float64)).reshape(N, rows, -1)
    if bias is not None:
        y = y + bias.astype(np.float64)
    return _act64(y, act)


@functools.lru_cache(maxsize=None)
def data(name):
    """-> dict(case, graph, x, w, bias, dy (gradients), ref): float32 inputs, the float64 reference of the case's output."""
    case = BY_NAME[name]
    g = graph(case.graph)
    rows, n_cols = g["out_rows"], g["n_cols"]
    rng = np.random.default_rng(sum(map(ord, name)))
    x = rng.standard_normal((case.N, n_cols, case.Fin)).astype(np.float32)
    d = {"case": case, "graph": g, "x": x, "w": None, "bias": None, "dy": None}
    if case.kind == "planes":
        fn = orc.chebyshev_planes if case.basis == "chebyshev" else orc.monomial_planes
        d["ref"] = fn(g["Lt"], x, case.K)[1:]
        return d
    if case.kind == "wgrad":
        d["dy"] = rng.standard_normal((case.N, rows, case.Fout)).astype(np.float32)
        planes = orc.chebyshev_planes(g["Lt"], x, case.K) if case.basis == "chebyshev" else orc.monomial_planes(g["Lt"], x, case.K)
        d["planes"] = planes.astype(np.float32)  # (for dsph_cheb_wgrad alone: the planes as the step kernels would hand them over)
        d["ref"] = np.ascontiguousarray(planes.transpose(3, 0, 1, 2)).reshape(case.Fin * case.K, -1) @ d["dy"].astype(np.float64).reshape(-1, case.Fout)
        return d
    d["w"] = (rng.standard_normal((case.Fin * case.K, case.Fout)) * orc.default_kernel_stddev(case.Fin, case.K)).astype(np.float32)
    d["bias"] = rng.standard_normal(case.Fout).astype(np.float32) if case.bias else None
    if case.kind == "parts":  # a shard's output rows are the whole sphere's forward on the rank's own rows [a, b)
        whole = rng.standard_normal((case.N, g["whole_Lt"].shape[0], case.Fin)).astype(np.float32)
        d["x"] = np.ascontiguousarray(whole[:, g["local_ids"]])
        a, b = g["own"]
        d["ref"] = _forward64(g["whole_Lt"], whole, d["w"], case.K, case.basis, d["bias"], case.act, g["whole_Lt"].shape[0])[:, a:b]
        return d
    y = _forward64(g["Lt"], x, d["w"], case.K, case.basis, d["bias"], case.act, rows)
    d["ref"] = orc.healpy_pool(y, 1, "MAX") if case.kind == "pool" else y
    return d


def out_shape(case, g=None):
    """Shape of the case's output, from the table alone (with the graph's sizes)."""
    g = g or graph(case.graph)
    rows, n_cols = g["out_rows"], g["n_cols"]
    if case.kind == "planes":
        return (case.K - 1, case.N, n_cols, case.Fin)
    if case.kind == "wgrad":
        return (case.Fin * case.K, case.Fout)
    if case.kind == "pool":
        return (case.N, rows // 4, case.Fout)
    return (case.N, rows, case.Fout)
