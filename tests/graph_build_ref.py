"""Reference side of the device graph build (not collected by pytest): brute-force k nearest pixels in float64, the validity rule
of a k-NN selection on HEALPix, the host formulas of ``healpix.healpix_graph`` / ``healpix_laplacian`` applied to a GIVEN selection,
and sentinel-guarded outputs for ``_native.healpix_knn``.

Ties.  HEALPix has mirror pairs of pixels at exactly the same distance from a third, so the k-th neighbour is often tied with the
(k+1)-th (nside 16, k = 60: 832 of 3072 rows within 1e-9 relative), and either member of the pair is a correct choice; the smallest
gap that is not such a tie was measured >= 8e-6 relative.  A selection is VALID for row i when, with d_k the true k-th smallest
distance and EPS = 1e-9: every chosen j has d(i, j) <= d_k (1 + EPS), and every pixel not chosen has d >= d_k (1 - EPS).  No test
demands equality with ``healpix_graph(mode="knn")``."""

import numpy as np
import torch
from scipy import sparse

from deepsphere import healpix

EPS = 1e-9          # the separator between a tie and a gap (measured: ties below 1e-9, gaps from 8e-6)
D2_RTOL = 1e-11     # d2 against the host's value: coordinates carry ~2^-52 absolute error, the smallest chords here are ~1e-2


def vectors(nside, indices=None):
    return healpix.pix2vec(nside, None if indices is None else np.asarray(indices, dtype=np.int64))


def brute_d2(vec, rows=None, block=1024):
    """Squared chords from the pixels ``rows`` (default all) to every pixel: float64 [len(rows), M], the host's expression
    sum((v_j - v_i)^2); the pixel itself at +inf."""
    M = vec.shape[0]
    rows = np.arange(M) if rows is None else np.asarray(rows)
    out = np.empty((rows.shape[0], M))
    for a in range(0, rows.shape[0], block):
        r = rows[a:a + block]
        out[a:a + block] = ((vec[None, :, :] - vec[r][:, None, :]) ** 2).sum(axis=2)
        out[np.arange(a, a + r.shape[0]), r] = np.inf
    return out


def brute_knn(vec, k, rows=None):
    """-> (nbr int64 [n, k] ascending by (d2, row), d2 [n, k], d2 of the (k+1)-th [n] (inf when there is none))."""
    D = brute_d2(vec, rows)
    order = np.argsort(D, axis=1, kind="stable")  # (stable: equal distances by ascending row)
    nbr = order[:, :k]
    d2 = np.take_along_axis(D, nbr, axis=1)
    nxt = np.take_along_axis(D, order[:, k:k + 1], axis=1)[:, 0] if D.shape[1] > k + 1 else np.full(D.shape[0], np.inf)
    return nbr, d2, nxt


def untied_rows(d2, nxt):
    """Rows whose (k+1)-th distance is clear of the k-th: the rows on which every correct k-NN search returns the same set."""
    return np.sqrt(nxt) > np.sqrt(d2[:, -1]) * (1 + 1e-6)


def selection_errors(vec, nbr, d2, rows=None, D=None):
    """The validity rule above on the rows ``rows`` (default all) of a selection (nbr [n, k], d2 [n, k] numpy): -> list of
    messages, empty when every row is valid, ascending by (d2, row), free of repeats and of the row itself, with d2 within D2_RTOL."""
    M = vec.shape[0]
    rows = np.arange(M) if rows is None else np.asarray(rows)
    nbr = np.asarray(nbr, dtype=np.int64)
    n, k = nbr.shape
    if D is None:
        D = brute_d2(vec, rows)
    errs = []
    if nbr.min() < 0 or nbr.max() >= M:
        return [f"neighbour rows outside [0, {M})"]
    if np.any(nbr == rows[:, None]):
        errs.append("a row lists itself")
    s = np.sort(nbr, axis=1)
    if np.any(s[:, 1:] == s[:, :-1]):
        errs.append("a row lists a pixel twice")
    true = np.take_along_axis(D, nbr, axis=1)
    rel = np.abs(d2 - true) / true
    if not np.all(rel <= D2_RTOL):
        errs.append(f"d2 off the host's value by {np.nanmax(rel):.3g} relative (allowed {D2_RTOL})")
    asc = (d2[:, 1:] > d2[:, :-1]) | ((d2[:, 1:] == d2[:, :-1]) & (nbr[:, 1:] > nbr[:, :-1]))
    if not np.all(asc):
        errs.append(f"{int((~asc).any(axis=1).sum())} rows do not ascend by (d2, row)")
    dk = np.sqrt(np.partition(D, k - 1, axis=1)[:, k - 1])
    if not np.all(np.sqrt(true) <= dk[:, None] * (1 + EPS)):
        errs.append(f"{int((np.sqrt(true) > dk[:, None] * (1 + EPS)).any(axis=1).sum())} rows chose a pixel beyond the k-th distance")
    rest = D.copy()
    np.put_along_axis(rest, nbr, np.inf, axis=1)
    if not np.all(np.sqrt(rest.min(axis=1)) >= dk * (1 - EPS)):
        errs.append(f"{int((np.sqrt(rest.min(axis=1)) < dk * (1 - EPS)).sum())} rows left out a pixel nearer than the k-th distance")
    return errs


def selection_errors_tree(vec, nbr, d2):
    """The same rule against ``cKDTree(k + 2)`` for maps too large for the distance matrix: the true k-th distance is the tree's;
    what the tree lists and the row did not choose must lie at d_k (1 - EPS) or beyond (anything the tree does not list lies at
    its (k+1)-th distance or beyond)."""
    from scipy.spatial import cKDTree

    M, k = nbr.shape
    nbr = np.asarray(nbr, dtype=np.int64)
    dist, ind = cKDTree(vec).query(vec, k=k + 2)
    keep = np.argsort(ind == np.arange(M)[:, None], axis=1, kind="stable")[:, :k + 1]  # (without the pixel itself)
    dist, ind = np.take_along_axis(dist, keep, axis=1), np.take_along_axis(ind, keep, axis=1)
    dk = np.sort(dist, axis=1)[:, k - 1]
    errs = []
    if np.any(nbr == np.arange(M)[:, None]):
        errs.append("a row lists itself")
    s = np.sort(nbr, axis=1)
    if np.any(s[:, 1:] == s[:, :-1]):
        errs.append("a row lists a pixel twice")
    true = ((vec[nbr] - vec[:, None, :]) ** 2).sum(axis=2)
    rel = np.abs(d2 - true) / true
    if not np.all(rel <= D2_RTOL):
        errs.append(f"d2 off the host's value by {np.nanmax(rel):.3g} relative")
    if not np.all((d2[:, 1:] > d2[:, :-1]) | ((d2[:, 1:] == d2[:, :-1]) & (nbr[:, 1:] > nbr[:, :-1]))):
        errs.append("rows do not ascend by (d2, row)")
    if not np.all(np.sqrt(true) <= dk[:, None] * (1 + EPS)):
        errs.append("a row chose a pixel beyond the k-th distance")
    for a in range(0, M, 4096):
        chosen = (ind[a:a + 4096, :, None] == nbr[a:a + 4096, None, :]).any(axis=2)
        if not np.all(chosen | (dist[a:a + 4096] >= dk[a:a + 4096, None] * (1 - EPS))):
            errs.append("a row left out a pixel nearer than the k-th distance")
            break
    return errs


def host_graph_from_selection(nbr, d2, kw):
    """``healpix.healpix_graph(mode="knn")`` behind its tree query, on a given selection: weights exp(-(d / kw)^2), max(A, A^T),
    zero diagonal, zeros eliminated, indices sorted (CSR float64)."""
    M, k = nbr.shape
    rows = np.repeat(np.arange(M, dtype=np.int64), k)
    w = np.exp(-((np.sqrt(np.asarray(d2, dtype=np.float64)).reshape(-1) / kw) ** 2))
    A = sparse.csr_matrix((w, (rows, np.asarray(nbr, dtype=np.int64).reshape(-1))), shape=(M, M))
    W = A.maximum(A.T).tocsr()
    W.setdiag(0.0)
    W.eliminate_zeros()
    W.sort_indices()
    return W


def host_laplacian_from_selection(nbr, d2, kw):
    """``healpix.healpix_laplacian`` on a given selection."""
    return healpix._normalized_laplacian(host_graph_from_selection(nbr, d2, kw))


BAND = 256


class GuardedKnn:
    """The three outputs of ``_native.healpix_knn`` as views inside larger allocations, a band of sentinels before and after each;
    the views are pre-filled with values no result holds (nbr -99, d2 NaN, ok 7)."""

    FILL = {torch.int32: (-77777, -99), torch.float64: (1e300, float("nan")), torch.uint8: (0xAB, 7)}

    def __init__(self, M, k, device="cuda"):
        self.bufs, views = [], []
        for dtype, shape in ((torch.int32, (M, k)), (torch.float64, (M, k)), (torch.uint8, (M,))):
            n = int(np.prod(shape))
            band, fill = self.FILL[dtype]
            buf = torch.full((n + 2 * BAND,), band, dtype=dtype, device=device)
            view = buf[BAND:BAND + n].view(shape)
            view.fill_(fill)
            self.bufs.append((buf, n, band))
            views.append(view)
        self.out = tuple(views)

    def check(self, what="healpix_knn"):
        for buf, n, band in self.bufs:
            touched = int((buf[:BAND] != band).sum()) + int((buf[BAND + n:] != band).sum())
            assert touched == 0, f"{what}: {touched} elements of the bands around a {buf.dtype} output were overwritten"
        nbr, d2, ok = self.out
        assert int((ok > 1).sum()) == 0, f"{what}: rows of ok were not written"
        good = ok == 1
        assert not bool(torch.isnan(d2[good]).any()) and int((nbr[good] == -99).sum()) == 0, f"{what}: an ok row was not written"
