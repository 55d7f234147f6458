#!/usr/bin/env python3
"""Drives the host-side plan builders of libdsphere (tile classification, class-T embedding, BFS ring tables, rectangle merge,
strip / quad-strip lists, tape split, shard levels, option changes) through the C ABI of the SANITIZER build
(`make -C deepsphere-cosmo-tf2_amd/csrc asan` -> build_asan/libdsphere_asan.so: host code under AddressSanitizer + UBSan on a stub
HIP runtime, no GPU).  Run with the sanitizer runtime preloaded (tests/test_host.py does):

    LD_PRELOAD=$(hipcc -print-file-name=libclang_rt.asan-x86_64.so) ASAN_OPTIONS=detect_leaks=0 python3 tools/asan/run_plan_builders.py

After the look-ups of a plan it calls the compute entry points (forward, pooled forward, planes, weight gradient) over every route
of the fused launch path: the stub drops the launches, so what runs under the sanitizers is the routing, the workspace layout and
the images bookkeeping.  DSPH_STUB_TRACE=<file> makes the stub record every launch, event record and wait in that file.

Prints one line per plan and per call, and "ASAN-DRIVER-OK" at the end; any sanitizer report aborts the process (non-zero exit).
numpy / scipy only: torch is not imported (its allocator and the preloaded sanitizer runtime do not mix)."""
import ctypes
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "deepsphere-cosmo-tf2_amd", "deepsphere")
pkg = types.ModuleType("deepsphere")  # the package without its __init__ (which imports the torch layers)
pkg.__path__ = [PKG]
sys.modules["deepsphere"] = pkg
from deepsphere import healpix, utils  # noqa: E402

LIB = ctypes.CDLL(os.path.join(ROOT, "deepsphere-cosmo-tf2_amd", "csrc", "build_asan", "libdsphere_asan.so"))
i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
LIB.dsph_plan_create.argtypes = [ctypes.POINTER(vp), i64, i64, i32, vp, vp, ctypes.c_int]
LIB.dsph_plan_destroy.argtypes = [vp]
LIB.dsph_plan_destroy.restype = None
LIB.dsph_plan_set_levels.argtypes = [vp, i32, vp]
LIB.dsph_plan_set_option.argtypes = [vp, i32, i64]
LIB.dsph_plan_prepare_layer.argtypes = [vp, i32, i32, i32, i32]
LIB.dsph_plan_tile_counts.argtypes = [vp, i32, ctypes.POINTER(i64), ctypes.POINTER(i64)]
LIB.dsph_plan_strip_tiles.argtypes = [vp, i64, i32, i32, i32, i32, ctypes.POINTER(i64)]
LIB.dsph_plan_strip_pairs.argtypes = [vp, i32, vp, i64, ctypes.POINTER(i64)]
LIB.dsph_plan_strip_split.argtypes = [vp, i64, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i64)]
LIB.dsph_plan_strip_rows.argtypes = [vp, i32, i64, i64, vp, vp]
LIB.dsph_plan_fused_ok.argtypes = [vp, i32, i32, i32]
LIB.dsph_workspace_bytes.argtypes = [vp, i64, i32, i32, i32, i32, i32]
LIB.dsph_workspace_bytes.restype = ctypes.c_size_t
LIB.dsph_backward_weights_workspace_bytes.argtypes = [vp, i64, i32, i32, i32, i32]
LIB.dsph_backward_weights_workspace_bytes.restype = ctypes.c_size_t
LIB.dsph_last_error.restype = ctypes.c_char_p
sz = ctypes.c_size_t
LIB.dsph_poly_forward_ex.argtypes = [vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, sz, vp]
LIB.dsph_poly_forward_pool.argtypes = [vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, i32, i32, i32, i32, vp, sz, vp]
LIB.dsph_cheb_planes.argtypes = [vp, vp, vp, i64, i32, i32, i32, i32, vp]
LIB.dsph_cheb_backward_weights.argtypes = [vp, vp, vp, vp, i64, i32, i32, i32, i32, i32, i32, vp, sz, vp]
LIB.dsph_stub_trace_note.argtypes = [ctypes.c_char_p]
LIB.dsph_stub_trace_note.restype = None


def ell_of(L, scale=0.75):
    Lt, _ = utils.prepare_L(L, scale=scale)
    cols, vals = utils.csr_to_ell(Lt)
    return np.ascontiguousarray(cols, np.int32), np.ascontiguousarray(vals, np.float32)


def plan_of(cols, vals, n_cols=None, levels=None, options=None):
    h = vp()
    rc = LIB.dsph_plan_create(ctypes.byref(h), cols.shape[0], cols.shape[0] if n_cols is None else n_cols, cols.shape[1],
                              cols.ctypes.data, vals.ctypes.data, 0)
    assert rc == 0, LIB.dsph_last_error()
    if levels is not None:
        lv = np.ascontiguousarray(levels, np.int64)
        assert LIB.dsph_plan_set_levels(h, len(lv), lv.ctypes.data) == 0, LIB.dsph_last_error()
    for k, v in (options or {}).items():
        assert LIB.dsph_plan_set_option(h, k, v) == 0, LIB.dsph_last_error()
    return h


def look(h, K, Fin, Fout, name, flags=1, N=(1, 3, 16)):
    assert LIB.dsph_plan_prepare_layer(h, K, Fin, Fout, flags) == 0, LIB.dsph_last_error()
    a, b, n = i64(0), i64(0), i64(0)
    rc = LIB.dsph_plan_tile_counts(h, K, ctypes.byref(a), ctypes.byref(b))
    ok = LIB.dsph_plan_fused_ok(h, Fin, Fout, K)
    strips = []
    for nn in N:
        t = i64(0)
        LIB.dsph_plan_strip_tiles(h, nn, Fin, Fout, K, 1, ctypes.byref(t))
        strips.append(t.value)
        LIB.dsph_workspace_bytes(h, nn, Fin, Fout, K, 1, 0)
        LIB.dsph_backward_weights_workspace_bytes(h, nn, Fin, Fout, K, 0)
        g, p, w, r = i32(0), i32(0), i32(0), i64(0)
        LIB.dsph_plan_strip_split(h, nn, ctypes.byref(g), ctypes.byref(p), ctypes.byref(w), ctypes.byref(r))
    LIB.dsph_plan_strip_pairs(h, K, None, 0, ctypes.byref(n))
    rec = np.zeros((max(n.value, 1), 12), np.int32)
    if n.value:
        assert LIB.dsph_plan_strip_pairs(h, K, rec.ctypes.data, n.value, ctypes.byref(n)) == 0
    print(f"{name}: K {K} {Fin}->{Fout}: tile_counts rc {rc} struct {a.value} bfs {b.value}, fused_ok {ok}, strip tiles {strips}, records {n.value}", flush=True)
    look.records = rec[: n.value]
    return a.value, b.value, strips


def check_strip_tables(h, K, cols, vals, name, D=4):
    """Every quad strip's table against the graph itself: a pixel's row, looked up through dsph_plan_strip_rows, must have its
    non-zeros of L~ exactly on the rows of the eight neighbouring pixels of the strip's plane (and itself) -- for every output
    pixel and every halo pixel a level is evaluated on (rings 0 .. D - 1 of the rectangle); output pixels are covered once."""
    rec = look.records
    seen = np.zeros(cols.shape[0], np.int32)
    for s, r in enumerate(rec):
        x0, w, y0, y1, xlo, xhi, ylo, yhi = int(r[0]), int(r[2]), int(r[6]), int(r[7]), int(r[8]), int(r[9]), int(r[10]), int(r[11])
        xa, xb = max(x0 - (D - 1), xlo + 1), min(x0 + w + (D - 1), xhi)  # evaluated columns of this strip (its neighbours cover the rest)
        ys = np.arange(ylo, yhi + 1)
        xs = np.arange(xa - 1, xb + 1)
        X, Y = np.meshgrid(xs, ys, indexing="ij")
        rows = np.zeros(X.size, np.int64)
        xy = np.ascontiguousarray(np.stack([X.ravel(), Y.ravel()], 1), np.int32)
        assert LIB.dsph_plan_strip_rows(h, K, s, xy.shape[0], xy.ctypes.data, rows.ctypes.data) == 0
        R = rows.reshape(X.shape)
        assert R.min() >= 0 and R.max() < cols.shape[0]
        inner = R[1:-1, 1:-1]                                          # rings 0 .. D - 1
        nb = np.stack([R[1 + dx: R.shape[0] - 1 + dx, 1 + dy: R.shape[1] - 1 + dy] for dx in (-1, 0, 1) for dy in (-1, 0, 1)], -1)
        c = cols[inner.ravel()]
        v = vals[inner.ravel()]
        ok = (v == 0) | (c[:, :, None] == nb.reshape(-1, 9)[:, None, :]).any(-1)
        assert ok.all(), f"{name}: strip {s}: a non-zero of L~ off the 3 x 3 window of the strip's plane"
        out = R[(x0 - (xa - 1)): (x0 - (xa - 1)) + w, (y0 - ylo): (y0 - ylo) + (y1 - y0)]
        np.add.at(seen, out.ravel(), 1)
        if K == 5:  # the rows a run of steps reads past the halo (the kernel does not clamp y): they must exist
            xs2, ys2 = np.arange(xlo, xhi + 1), np.concatenate([np.arange(ylo - 1, ylo), np.arange(yhi + 1, yhi + 7)])
            X2, Y2 = np.meshgrid(xs2, ys2, indexing="ij")
            xy2 = np.ascontiguousarray(np.stack([X2.ravel(), Y2.ravel()], 1), np.int32)
            rows2 = np.zeros(xy2.shape[0], np.int64)
            assert LIB.dsph_plan_strip_rows(h, K, s, xy2.shape[0], xy2.ctypes.data, rows2.ctypes.data) == 0
            assert rows2.min() >= 0 and rows2.max() < cols.shape[0], f"{name}: strip {s}: a row past the halo does not exist ({rows2.max()} of {cols.shape[0]})"
    assert seen.max() <= 1, f"{name}: an output pixel in two strips"
    print(f"{name}: {len(rec)} strips, {int(seen.sum())} output pixels = {int(seen.sum()) // 256} tiles, tables verified against the graph", flush=True)
    return int(seen.sum()) // 256


def shard_of(cols, vals, lo, hi, K):
    """Rows [lo, hi) of a graph as a plan with halo columns ordered by hop distance and a shrinking schedule (what
    deepsphere/sharding.ShardLayout builds, restated without torch)."""
    M, W = cols.shape
    dist = np.full(M, -1, np.int64)
    dist[lo:hi] = 0
    frontier = np.arange(lo, hi)
    order = [frontier]
    for d in range(1, K):
        nb = np.unique(cols[frontier][vals[frontier] != 0])
        nb = nb[dist[nb] < 0]
        dist[nb] = d
        order.append(nb)
        frontier = nb
    ids = np.concatenate(order)
    local = np.full(M, -1, np.int64)
    local[ids] = np.arange(ids.size)
    n_rows = int(sum(len(o) for o in order[: K - 1]))  # rows within K-2 hops carry a matrix row
    lc = local[cols[ids[:n_rows]]]
    lv = vals[ids[:n_rows]].copy()
    lv[lc < 0] = 0
    lc[lc < 0] = np.arange(n_rows)[:, None].repeat(W, 1)[lc < 0]
    levels = np.cumsum([len(o) for o in order[: K - 1]])
    return np.ascontiguousarray(lc, np.int32), np.ascontiguousarray(lv, np.float32), ids.size, levels


# ---- the launch path: the compute entry points on the stub runtime ---------------------------------------------------------------
# Launches are dropped, so x, w, y are never read: one small aligned buffer stands for all of them.  The workspace is a real
# allocation of exactly the size the library asks for.  Every call prints its return code and error text; with DSPH_STUB_TRACE
# set, the stub appends what the call launched (kernel, grid, block, stream; fork and join) under the call's name.
_DUMMY = np.zeros(1 << 12, np.uint8)
BUF = (_DUMMY.ctypes.data + 15) & ~15
OPT_STRIPS, OPT_STRUCT, OPT_TABLES, OPT_FORK, OPT_MINROWS, OPT_SPLIT, OPT_PACK, OPT_STRIP_FORM = 1, 2, 3, 4, 6, 8, 10, 11
PREC = {0: "fp32", 1: "bf16x3", 2: "bf16x6", 3: "f16x3"}
RELU, ELU, KEEP = 1, 2, 1


class Workspace:
    def __init__(self, nbytes):
        self.raw = np.empty(nbytes + 16, np.uint8)
        self.ptr = (self.raw.ctypes.data + 15) & ~15
        self.nbytes = nbytes


def report(name, rc):
    print(f"{name}: rc {rc}" + (f" [{LIB.dsph_last_error().decode()}]" if rc else ""), flush=True)
    return rc


def forward(h, name, N, Fin, Fout, K, prec=1, act=0, basis=0, part=0, flags=0, bias=False, ws=None, short=0, x_off=0, y_off=0, pool=None):
    """dsph_poly_forward_ex, or dsph_poly_forward_pool with pool = 0 (max) / 1 (mean); short: bytes withheld from the workspace;
    x_off, y_off: bytes by which x / y miss their 16-byte boundary (x: an error; y: the strips fall back to the tile kernels)."""
    need = LIB.dsph_workspace_bytes(h, N, Fin, Fout, K, prec, 0)
    ws = ws or Workspace(need)
    name = f"{name}: forward N {N} {Fin}->{Fout} K {K} {PREC[prec]} act {act} basis {basis} part {part} flags {flags} workspace {need}" + \
           (f" pool {pool}" if pool is not None else "") + (f" short {short}" if short else "") + (f" x+{x_off}" if x_off else "") + \
           (f" y+{y_off}" if y_off else "")
    LIB.dsph_stub_trace_note(name.encode())
    b = BUF if bias else None
    if pool is None:
        rc = LIB.dsph_poly_forward_ex(h, BUF + x_off, BUF, b, BUF + y_off, N, Fin, Fout, K, basis, act, prec, 0, part, flags, ws.ptr, ws.nbytes - short, None)
    else:
        rc = LIB.dsph_poly_forward_pool(h, BUF + x_off, BUF, b, BUF, BUF, N, Fin, Fout, K, basis, act, prec, pool, flags, ws.ptr, ws.nbytes - short, None)
    report(name, rc)
    return ws


def planes(h, name, N, Fin, K):
    name = f"{name}: planes N {N} Fin {Fin} K {K}"
    LIB.dsph_stub_trace_note(name.encode())
    report(name, LIB.dsph_cheb_planes(h, BUF, BUF, N, Fin, K, 0, 0, None))


def wgrad(h, name, N, Fin, Fout, K, prec=1, short=0):
    need = LIB.dsph_backward_weights_workspace_bytes(h, N, Fin, Fout, K, 0)
    ws = Workspace(need)
    name = f"{name}: weight gradient N {N} {Fin}->{Fout} K {K} {PREC[prec]} workspace {need}" + (f" short {short}" if short else "")
    LIB.dsph_stub_trace_note(name.encode())
    report(name, LIB.dsph_cheb_backward_weights(h, BUF, BUF, BUF, N, Fin, Fout, K, 0, prec, 0, ws.ptr, ws.nbytes - short, None))


def grid_launches(cols, vals, nside):
    """Every route of the launch path on the full-sphere grid: strips by cost rule / always / never in both forms, column
    blocks, deferred activation, kept weight images, padded and packed narrow layers, pooling, the K = 8 strips, K > 5."""
    for strips in (0, 1, 2):
        for form in (0, 1):
            name = f"launch grid nside {nside} strips {strips} form {form}"
            h = plan_of(cols, vals, options={OPT_STRIPS: strips, OPT_STRIP_FORM: form})
            for N in (1, 3, 16):
                for prec in (1, 3):
                    forward(h, name, N, 64, 64, 5, prec)
                forward(h, name, N, 64, 96, 5)
                forward(h, name, N, 64, 128, 5, bias=True, act=RELU)
                forward(h, name, N, 64, 64, 5, act=ELU, bias=True)
            forward(h, name, 3, 64, 64, 5, basis=1)
            forward(h, name, 16, 64, 64, 5, y_off=4)
            if form == 0:  # kept images: nothing packed by the second call, only the missing ones after strips <-> tiles
                ws = forward(h, name + " keep", 16, 64, 64, 5, flags=KEEP)
                forward(h, name + " keep", 16, 64, 64, 5, flags=KEEP, ws=ws)
                forward(h, name + " keep", 1, 64, 64, 5, flags=KEEP, ws=ws)
                wgrad(h, name, 16, 64, 64, 5)       # the quad-strip gradient + the rest on the BFS kernel, where the rule says so
                wgrad(h, name, 1, 64, 64, 5, prec=0)
            LIB.dsph_plan_destroy(h)
    name = f"launch grid nside {nside}"
    h = plan_of(cols, vals)
    for Fin in (1, 2, 3, 16):
        for Fout in (16, 32):
            for K in (3, 5):
                for prec in (0, 1, 2, 3):
                    forward(h, name, 4, Fin, Fout, K, prec, act=RELU, bias=True)
        forward(h, name, 1, Fin, 16, 5)
        for pool in (0, 1):
            forward(h, name, 4, Fin, 16, 5, act=RELU, pool=pool)
    ws = forward(h, name + " keep", 4, 4, 16, 5, flags=KEEP)
    forward(h, name + " keep", 1, 4, 16, 5, flags=KEEP, ws=ws)  # (a single map is not packed: other images)
    forward(h, name, 4, 8, 32, 5)
    wgrad(h, name, 4, 128, 64, 5)
    wgrad(h, name, 4, 16, 32, 5)
    wgrad(h, name, 4, 1, 16, 5)
    planes(h, name, 2, 16, 5)
    forward(h, name, 1, 64, 64, 5, short=1)
    forward(h, name, 2, 1, 16, 5, short=1)
    wgrad(h, name, 2, 64, 64, 5, short=1)
    forward(h, name, 1, 64, 64, 5, x_off=4)
    forward(h, name, 4, 4, 16, 5, y_off=4)
    forward(h, name, 1, 64, 64, 5, act=ELU, pool=0)   # no fused pooling: the activation
    if nside == 128:
        for strips in (0, 2):
            assert LIB.dsph_plan_set_option(h, OPT_STRIPS, strips) == 0
            for N in (1, 16):
                forward(h, name + f" strips {strips}", N, 32, 32, 8, act=RELU, bias=True)
                forward(h, name + f" strips {strips}", N, 32, 32, 8, prec=3)
            forward(h, name + f" strips {strips}", 2, 32, 32, 8, act=ELU)
            forward(h, name + f" strips {strips}", 16, 32, 32, 8, y_off=4)
    else:
        forward(h, name, 2, 32, 32, 8)        # 7-ring BFS tables
        forward(h, name, 2, 16, 32, 10)       # the 1168-row variant
        forward(h, name, 2, 32, 32, 12)
        assert LIB.dsph_plan_set_option(h, OPT_SPLIT, 1) == 0
        forward(h, name + " split", 2, 16, 32, 10)  # the chain of passes
        ws = forward(h, name + " split keep", 2, 16, 32, 10, flags=KEEP)
        forward(h, name + " split keep", 2, 16, 32, 10, flags=KEEP, ws=ws)
    LIB.dsph_plan_destroy(h)
    if nside == 64:
        for opt in (OPT_STRUCT, OPT_TABLES, OPT_FORK, OPT_PACK):
            h = plan_of(cols, vals, options={opt: 0})
            forward(h, f"launch grid nside {nside} option {opt}=0", 4, 64, 64, 5)
            forward(h, f"launch grid nside {nside} option {opt}=0", 4, 4, 16, 5)
            LIB.dsph_plan_destroy(h)
        h = plan_of(cols, vals, options={OPT_STRIPS: 1})
        forward(h, f"launch grid nside {nside} strips 1", 4, 64, 64, 5, act=RELU, pool=0)  # no fused pooling: the strips' shape
        LIB.dsph_plan_destroy(h)


def main():
    # full-sphere grid stencil: class R interiors (strips at 64 -> 64), class T face borders, class G corners
    for nside in (32, 64, 128):
        cols, vals = ell_of(healpix.healpix_laplacian(nside, mode="grid"))
        h = plan_of(cols, vals, options={OPT_STRIPS: 1})
        s, b, st = look(h, 5, 64, 64, f"grid nside {nside}")
        assert s + b == cols.shape[0] // 256 and b == 24
        if st[0]:
            assert check_strip_tables(h, 5, cols, vals, f"grid nside {nside}") == st[0]
        look(h, 5, 16, 32, f"grid nside {nside}")
        look(h, 3, 1, 16, f"grid nside {nside}")
        if nside == 128:  # the K = 8, 32 -> 32 quad strips: rectangles of the tiles whose 7-ring region stays inside a base pixel
            _, _, st8 = look(h, 8, 32, 32, f"grid nside {nside}")
            assert st8[0] >= 12 * 36 and check_strip_tables(h, 8, cols, vals, f"grid nside {nside} K 8", D=7) == st8[0]
        if nside == 64:
            look(h, 8, 32, 32, f"grid nside {nside}")          # 7-ring BFS tables
            look(h, 10, 16, 32, f"grid nside {nside}")         # the chain of passes
            for opt, v in ((OPT_STRIP_FORM, 1), (OPT_TABLES, 0), (OPT_STRUCT, 0), (OPT_SPLIT, 1), (OPT_MINROWS, 6)):
                assert LIB.dsph_plan_set_option(h, opt, v) == 0  # drops the tables: rebuilt below
                look(h, 5, 64, 64, f"grid nside {nside} option {opt}={v}")
            assert LIB.dsph_plan_set_option(h, 99, 0) != 0
        look(h, 5, 64, 64, f"grid nside {nside} release", flags=3)  # DSPH_PREPARE_RELEASE_HOST: further K fail cleanly
        assert LIB.dsph_plan_prepare_layer(h, 4, 64, 64, 0) in (0, -3)
        LIB.dsph_plan_destroy(h)
        if nside >= 64:
            grid_launches(cols, vals, nside)
    # partial sky: a cap padded to superpixels (ragged rectangles, compacted rows: class T rings around every superpixel)
    for nside, sup in ((64, 8), (128, 8), (64, 2)):
        idx = healpix.extend_indices(healpix.cap_indices(nside, fraction=1.0 / 3.0), nside, sup)
        cols, vals = ell_of(healpix.healpix_laplacian(nside, indices=idx, mode="grid"))
        h = plan_of(cols, vals, options={OPT_STRIPS: 1})
        _, _, st = look(h, 5, 64, 64, f"cap nside {nside} superpixels {sup} ({cols.shape[0]} rows)")
        if st[0]:
            assert check_strip_tables(h, 5, cols, vals, f"cap nside {nside} superpixels {sup}") == st[0]
        LIB.dsph_plan_destroy(h)
        if nside == 64:
            h = plan_of(cols, vals)
            for N in (1, 16):
                forward(h, f"launch cap superpixels {sup}", N, 64, 64, 5)
            wgrad(h, f"launch cap superpixels {sup}", 16, 64, 64, 5)
            LIB.dsph_plan_destroy(h)
    # the reference's graphs: k nearest neighbours (ELL width 11: BFS tiles; 23: the tiled step's depth-1 tables)
    for k in (8, 20):
        cols, vals = ell_of(healpix.healpix_laplacian(32, n_neighbors=k, mode="knn"))
        h = plan_of(cols, vals)
        look(h, 5, 16, 32, f"knn{k} nside 32 (width {cols.shape[1]})")
        forward(h, f"launch knn{k}", 2, 16, 32, 5)  # (k = 20: no fused kernel, the tiled step)
        if k == 8:
            planes(h, f"launch knn{k}", 2, 16, 5)
        LIB.dsph_plan_destroy(h)
    # a shard: half the sphere with its (K-1)-ring halo as trailing columns and a shrinking schedule
    cols, vals = ell_of(healpix.healpix_laplacian(64, mode="grid"))
    M = cols.shape[0]
    for K in (5, 8):
        for lo, hi in ((0, M // 2), (M // 4, M // 2), (M - M // 8, M)):
            lc, lv, n_cols, levels = shard_of(cols, vals, lo, hi, K)
            h = plan_of(lc, lv, n_cols=n_cols, levels=levels)
            look(h, K, 32, 32, f"shard rows [{lo}, {hi}) K {K}: {lc.shape[0]} rows, {n_cols} columns")
            for part in (0, 1, 2):
                for act in (RELU, ELU):
                    forward(h, f"launch shard [{lo}, {hi})", 2, 32, 32, K, act=act, bias=True, part=part)
            if K == 5:
                planes(h, f"launch shard [{lo}, {hi})", 2, 32, K)
                wgrad(h, f"launch shard [{lo}, {hi})", 2, 32, 32, K)
            LIB.dsph_plan_destroy(h)
            if K == 5 and lo == 0:  # the schedule's errors: none at all, too short
                for bad, what in ((None, "no levels"), (levels[:2], "two levels")):
                    h = plan_of(lc, lv, n_cols=n_cols, levels=bad)
                    forward(h, f"launch shard with {what}", 2, 32, 32, K)
                    planes(h, f"launch shard with {what}", 2, 32, K)
                    wgrad(h, f"launch shard with {what}", 2, 32, 32, K)
                    LIB.dsph_plan_destroy(h)
    # a map whose last tile is incomplete, with strips: no rectangle may have that tile in its ring (the kernel reads rows of the
    # ring tiles past the halo)
    M = 12 * 64 * 64
    for drop in (100, 200, 256 + 37):
        cols, vals = ell_of(healpix.healpix_laplacian(64, indices=np.arange(M - drop), mode="grid"))
        h = plan_of(cols, vals, options={OPT_STRIPS: 1})
        _, _, st = look(h, 5, 64, 64, f"grid nside 64 without its last {drop} pixels ({cols.shape[0]} rows)")
        assert st[0] > 0 and check_strip_tables(h, 5, cols, vals, f"grid nside 64 without its last {drop} pixels") == st[0]
        LIB.dsph_plan_destroy(h)
    # a ragged tail (rows not a multiple of 256) and a tiny graph
    cols, vals = ell_of(healpix.healpix_laplacian(8, mode="grid"))
    h = plan_of(cols[:700].clip(max=699), vals[:700])
    look(h, 5, 4, 8, "ragged 700 rows")
    LIB.dsph_plan_destroy(h)
    print("ASAN-DRIVER-OK", flush=True)


if __name__ == "__main__":
    main()
