"""Reference side of the device build of HealpySmoothing's kernel table (not collected by pytest): the validity rule of a table
row under HEALPix's ties, brute-force disc counts, a brute-force stand-in for the two ``_native`` calls, sentinel-guarded outputs
and the pixel sets of the tests.

Ties.  The W-th neighbour of a pixel is often tied with the (W+1)-th (mirror pairs of pixels), so no test demands the host's
table.  A row is VALID when, with d_W the true W-th smallest distance (the pixel itself included) and EPS = 1e-9 (the separator of
tests/graph_build_ref.py): it holds W distinct columns in [0, M), ascending; every pixel nearer than d_W (1 - EPS) is present; every
listed pixel lies within d_W (1 + EPS); ``vals`` equals kern / sum(kern) on the listed columns to rtol 1e-6; |sum(vals) - 1| <=
W 2^-24 (both from tests/test_smoothing_host.py)."""

import functools

import numpy as np
import torch

import smoothing_ref as ref
from deepsphere import healpix
from graph_build_ref import BAND, EPS

VALS_RTOL = 1e-6


def res(nside):
    """Pixel resolution: the square root of the pixel area."""
    return np.sqrt(4 * np.pi / (12 * nside * nside))


def radius(sigma_rad, n_sigma):
    return min(float(sigma_rad) * float(n_sigma), np.pi)


def chord2(rho):
    """Squared chord of the angle ``rho``: the ``r2`` of ``_native.healpix_disc_count``."""
    return float((2.0 * np.sin(0.5 * rho)) ** 2)


def cap16():
    return healpix.extend_indices(healpix.cap_indices(16, fraction=1 / 3), 16, 4)


def ragged32():
    """A random 30 % of the nside-8 super-pixels, at nside 32 (the set of tests/test_gpu_graph_build.py)."""
    parents = np.sort(np.random.default_rng(5).choice(768, size=230, replace=False))
    return (parents[:, None] * 16 + np.arange(16)[None, :]).reshape(-1).astype(np.int64)


SETS = {"full": lambda nside: np.arange(12 * nside * nside, dtype=np.int64), "cap16": lambda nside: cap16(),
        "ragged32": lambda nside: ragged32()}


class Brute:
    """All pairs of one case, computed once: ``theta`` [M, M], ``W``, ``d_k`` [M], ``kern`` [M, M], ``counts`` [M] (pixels within
    the disc, the pixel itself included)."""

    def __init__(self, nside, indices, sigma_rad, n_sigma):
        self.nside, self.indices, self.sigma_rad, self.n_sigma = nside, np.asarray(indices, dtype=np.int64), sigma_rad, n_sigma
        self.theta, self.W, self.d_k, self.kern = ref.brute_table(nside, self.indices, sigma_rad, n_sigma)
        self.rho = radius(sigma_rad, n_sigma)
        self.counts = (self.theta <= self.rho).sum(axis=1)
        self.M = self.theta.shape[0]


@functools.lru_cache(maxsize=4)
def brute(nside, which, sigma_over_res, n_sigma):
    return Brute(nside, SETS[which](nside), sigma_over_res * res(nside), n_sigma)


def table_errors(b, cols, vals, rows=None):
    """The validity rule on the rows ``rows`` (default all) of a table (cols, vals numpy [n, W]) against the all-pairs case ``b``:
    -> list of messages, empty when every row is valid."""
    rows = np.arange(b.M) if rows is None else np.asarray(rows)
    cols, vals = np.asarray(cols), np.asarray(vals)
    n, W = cols.shape
    errs = []
    if W != b.W:
        return [f"rows of {W} entries, brute force has W = {b.W}"]
    if n != rows.shape[0] or vals.shape != cols.shape:
        return ["table and rows differ in shape"]
    if n == 0:
        return errs
    if cols.min() < 0 or cols.max() >= b.M:
        return [f"columns outside [0, {b.M})"]
    c = cols.astype(np.int64)
    if not np.all(c[:, 1:] > c[:, :-1]):
        dup = np.sort(c, axis=1)
        what = "a row lists a pixel twice" if np.any(dup[:, 1:] == dup[:, :-1]) else "columns of a row do not ascend"
        errs.append(what)
    theta = b.theta[rows]
    d_k = b.d_k[rows]
    listed = np.take_along_axis(theta, c, axis=1)
    if not np.all(listed <= d_k[:, None] * (1 + EPS)):
        errs.append(f"{int((listed > d_k[:, None] * (1 + EPS)).any(axis=1).sum())} rows list a pixel beyond the W-th distance")
    rest = theta.copy()
    np.put_along_axis(rest, c, np.inf, axis=1)
    if not np.all(rest.min(axis=1) >= d_k * (1 - EPS)):
        errs.append(f"{int((rest.min(axis=1) < d_k * (1 - EPS)).sum())} rows leave out a pixel nearer than the W-th distance")
    kern = np.take_along_axis(b.kern[rows], c, axis=1)
    want = kern / kern.sum(axis=1, keepdims=True)
    rel = np.abs(vals.astype(np.float64) - want) / want
    if not np.all(rel <= VALS_RTOL):
        errs.append(f"vals off kern / sum(kern) by {np.nanmax(rel):.3g} relative (allowed {VALS_RTOL})")
    off = np.abs(vals.astype(np.float64).sum(axis=1) - 1.0).max()
    if not off <= W * 2.0**-24:
        errs.append(f"a row sums to 1 +- {off:.3g} (allowed {W * 2.0**-24:.3g})")
    return errs


def table_errors_tree(nside, indices, sigma_rad, cols, vals, rows):
    """The same rule on the rows ``rows`` of a table too large for all pairs, against ``cKDTree(k = W + 2)`` in the manner of
    ``graph_build_ref.selection_errors_tree``: the true W-th distance is the tree's; what the tree lists and the row does not must
    lie at d_W (1 - EPS) or beyond (anything the tree does not list lies at its (W+1)-th distance or beyond)."""
    from scipy.spatial import cKDTree

    vec = healpix.pix2vec(nside, None if indices is None else np.asarray(indices, dtype=np.int64))
    rows = np.asarray(rows)
    c = np.asarray(cols)[rows].astype(np.int64)
    v = np.asarray(vals)[rows].astype(np.float64)
    n, W = c.shape
    M = vec.shape[0]
    errs = []
    if c.min() < 0 or c.max() >= M:
        return [f"columns outside [0, {M})"]
    if not np.all(c[:, 1:] > c[:, :-1]):
        errs.append("columns of a row do not ascend strictly")
    dist, ind = cKDTree(vec).query(vec[rows], k=W + 2)
    d_k = np.sort(dist, axis=1)[:, W - 1]  # (chords: monotone in the angle)
    own = np.sqrt(((vec[c] - vec[rows][:, None, :]) ** 2).sum(axis=2))
    if not np.all(own <= d_k[:, None] * (1 + EPS)):
        errs.append("a row lists a pixel beyond the W-th distance")
    for a in range(0, n, 512):
        chosen = (ind[a:a + 512, :, None] == c[a:a + 512, None, :]).any(axis=2)
        if not np.all(chosen | (dist[a:a + 512] >= d_k[a:a + 512, None] * (1 - EPS))):
            errs.append("a row leaves out a pixel nearer than the W-th distance")
            break
    theta = 2.0 * np.arcsin(np.minimum(0.5 * own, 1.0))
    kern = np.exp(-0.5 * (theta / sigma_rad) ** 2)
    want = kern / kern.sum(axis=1, keepdims=True)
    rel = np.abs(v - want) / want
    if not np.all(rel <= VALS_RTOL):
        errs.append(f"vals off kern / sum(kern) by {np.nanmax(rel):.3g} relative (allowed {VALS_RTOL})")
    off = np.abs(v.sum(axis=1) - 1.0).max()
    if not off <= W * 2.0**-24:
        errs.append(f"a row sums to 1 +- {off:.3g} (allowed {W * 2.0**-24:.3g})")
    return errs


def brute_rows(b, rows=None):
    """The rows ``rows`` of the table of case ``b`` by brute force, selected by (theta, row) ascending, in the layout of
    ``_native.healpix_gauss_table``: -> (cols int32, vals float32, raw float32), every row ascending by column."""
    rows = np.arange(b.M) if rows is None else np.asarray(rows)
    order = np.argsort(b.theta[rows], axis=1, kind="stable")[:, :b.W]
    cols = np.sort(order, axis=1)
    raw = np.take_along_axis(b.kern[rows], cols, axis=1).astype(np.float32)
    vals = (raw / raw.sum(axis=1, dtype=np.float64, keepdims=True)).astype(np.float32)
    return cols.astype(np.int32), vals, raw


class FakeNative:
    """Stand-ins for ``_native.healpix_disc_count`` / ``_native.healpix_gauss_table`` on CPU tensors: brute-force results of case
    ``b``, with the rows ``flag_count`` / ``flag_table`` flagged and filled with rubbish, as a kernel may leave them."""

    def __init__(self, b, flag_count=(), flag_table=()):
        self.b, self.flag_count, self.flag_table = b, np.asarray(flag_count, dtype=np.int64), np.asarray(flag_table, dtype=np.int64)
        self.calls = []

    def healpix_disc_count(self, nside, r2, indices=None, lut=None, device=None, out=None):
        self.calls.append("count")
        assert nside == self.b.nside and abs(r2 - chord2(self.b.rho)) <= 1e-15
        count = torch.as_tensor(self.b.counts.astype(np.int32))
        ok = torch.ones(self.b.M, dtype=torch.uint8)
        count[self.flag_count] = 0
        ok[self.flag_count] = 0
        return count, ok

    def healpix_gauss_table(self, nside, W, sigma_rad, rho, indices=None, lut=None, device=None, want_raw=False, out=None):
        self.calls.append("table")
        assert W == self.b.W and sigma_rad == self.b.sigma_rad
        cols, vals, raw = (torch.as_tensor(t.copy()) for t in brute_rows(self.b))
        ok = torch.ones(self.b.M, dtype=torch.uint8)
        cols[self.flag_table] = -1
        vals[self.flag_table] = 7.0
        raw[self.flag_table] = 7.0
        ok[self.flag_table] = 0
        return cols, vals, (raw if want_raw else None), ok


class Guarded:
    """Tensors of the given (dtype, shape) as views inside larger allocations, a band of sentinels before and after each; the
    views are pre-filled with values no result holds (int32 -99, float32 NaN, uint8 7), as ``graph_build_ref.GuardedKnn`` does."""

    FILL = {torch.int32: (-77777, -99), torch.float32: (1e30, float("nan")), torch.uint8: (0xAB, 7)}

    def __init__(self, specs, device="cuda"):
        self.bufs, views = [], []
        for dtype, shape in specs:
            n = int(np.prod(shape))
            band, fill = self.FILL[dtype]
            buf = torch.full((n + 2 * BAND,), band, dtype=dtype, device=device)
            view = buf[BAND:BAND + n].view(shape)
            view.fill_(fill)
            self.bufs.append((buf, n, band, fill))
            views.append(view)
        self.out = tuple(views)

    def check(self, what):
        for buf, n, band, fill in self.bufs:
            touched = int((buf[:BAND] != band).sum()) + int((buf[BAND + n:] != band).sum())
            assert touched == 0, f"{what}: {touched} elements of the bands around a {buf.dtype} output were overwritten"
            body = buf[BAND:BAND + n]
            unwritten = int(torch.isnan(body).sum()) if buf.dtype == torch.float32 else int((body == fill).sum())
            assert unwritten == 0, f"{what}: {unwritten} elements of a {buf.dtype} output were not written"


def scipy_transposed(cols, vals):
    """``HealpySmoothing._transposed_tables`` on a given table (numpy): the scipy route."""
    from scipy import sparse

    M, W = cols.shape
    K = sparse.csr_matrix((vals.reshape(-1).copy(), cols.reshape(-1).copy(), np.arange(0, M * W + 1, W)), shape=(M, M))
    K.eliminate_zeros()  # (in place: hence the copies)
    KT = K.T.tocsr()
    KT.sort_indices()
    lens = np.diff(KT.indptr)
    WT = max(int(lens.max()), 1)
    colsT = np.repeat(np.arange(M, dtype=np.int32)[:, None], WT, axis=1)
    valsT = np.zeros((M, WT), dtype=np.float32)
    slot = np.arange(KT.nnz) - np.repeat(KT.indptr[:-1], lens)
    r = np.repeat(np.arange(M), lens)
    colsT[r, slot] = KT.indices
    valsT[r, slot] = KT.data
    return colsT, valsT
