"""HEALPix geometry (NEST, and the RING <-> NEST index maps) and graph-Laplacian producer (host side, numpy/scipy only).

The reference obtains its Laplacians from two third-party packages that exist on
neither box (healpy, and the ``SphereHealpix`` class of a pygsp fork):
``healpy_networks.py:110-118`` calls ``SphereHealpix(subdivisions=nside,
indexes=indices, nest=True, k=n_neighbors, lap_type="normalized").L``.  This module
produces Laplacians of the same family from the published HEALPix algorithm
(Gorski et al. 2005): pixel centres, the 8 grid neighbours of a pixel, and two
graph builders (symmetrised k-NN with a Gaussian kernel, and the fixed 8-neighbour
grid stencil of the north-star text).  The convolution never depends on *how* L was
produced (L is an input of the layer, ``gnn_layers.py:17``), so nothing here is on
the parity path; it only feeds tests and the benchmark with realistic matrices.

The last part of the module builds the same graphs on the device (``healpix_graph_device``, ``healpix_laplacian_ell``,
``healpix_adjacency_tables``): neighbours from the HIP kernel ``dsph_healpix_knn``, the rest as torch operators; and the kernel
table of ``HealpySmoothing`` (``gauss_table_device``, ``transpose_table``) from the kernels of ``csrc/healpix_disc.hip``.
"""

import numpy as np
from scipy import sparse

__all__ = [
    "nside2npix",
    "npix2nside",
    "isnsideok",
    "nest2xyf",
    "xyf2nest",
    "nest2ring",
    "ring2nest",
    "reorder",
    "reorder_table",
    "pix2vec",
    "ang2pix",
    "vec2pix",
    "pix2ang",
    "get_interp_weights",
    "get_interp_val",
    "rotation_matrix",
    "random_rotations",
    "rotation_stencil",
    "alm_size",
    "alm_index",
    "legendre_lambda",
    "map2alm",
    "alm2map",
    "alm2cl",
    "anafast",
    "almxfl",
    "neighbours",
    "kernel_width",
    "healpix_graph",
    "healpix_laplacian",
    "grid_laplacian_ell",
    "grid_laplacian_ell_torch",
    "healpix_knn_device",
    "DeviceGraph",
    "healpix_graph_device",
    "healpix_laplacian_ell",
    "healpix_adjacency_tables",
    "gauss_table_device",
    "transpose_table",
    "cap_indices",
    "extend_indices",
    "superpixel_padding_mask",
]

# base-pixel ("face") ring/phi offsets of the HEALPix projection
_JRLL = np.array([2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4], dtype=np.int64)
_JPLL = np.array([1, 3, 5, 7, 0, 2, 4, 6, 1, 3, 5, 7], dtype=np.int64)

# neighbour direction order: SW, W, NW, N, NE, E, SE, S
_NB_XOFF = np.array([-1, -1, 0, 1, 1, 1, 0, -1], dtype=np.int64)
_NB_YOFF = np.array([0, 1, 1, 1, 0, -1, -1, -1], dtype=np.int64)
# which face a step off the edge of a face lands in; row = 3*(dy+1) + (dx+1), -1: no face
_NB_FACE = np.array(
    [
        [8, 9, 10, 11, -1, -1, -1, -1, 10, 11, 8, 9],  # S
        [5, 6, 7, 4, 8, 9, 10, 11, 9, 10, 11, 8],  # SE
        [-1, -1, -1, -1, 5, 6, 7, 4, -1, -1, -1, -1],  # E
        [4, 5, 6, 7, 11, 8, 9, 10, 11, 8, 9, 10],  # SW
        [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11],  # centre
        [1, 2, 3, 0, 0, 1, 2, 3, 5, 6, 7, 4],  # NE
        [-1, -1, -1, -1, 7, 4, 5, 6, -1, -1, -1, -1],  # W
        [3, 0, 1, 2, 3, 0, 1, 2, 4, 5, 6, 7],  # NW
        [2, 3, 0, 1, -1, -1, -1, -1, 0, 1, 2, 3],  # N
    ],
    dtype=np.int64,
)
# coordinate fix-up when crossing into that face, indexed [row][face >> 2]:
# bit0 flip x, bit1 flip y, bit2 swap x and y
_NB_SWAP = np.array(
    [[0, 0, 3], [0, 0, 6], [0, 0, 0], [0, 0, 5], [0, 0, 0], [5, 0, 0], [0, 0, 0], [6, 0, 0], [3, 0, 0]],
    dtype=np.int64,
)


def nside2npix(nside):
    return 12 * int(nside) * int(nside)


def isnsideok(nside):
    nside = int(nside)
    return nside > 0 and (nside & (nside - 1)) == 0


def npix2nside(npix):
    nside = int(round(np.sqrt(npix / 12.0)))
    if 12 * nside * nside != npix:
        raise ValueError(f"{npix} is not a valid HEALPix pixel count")
    return nside


def _compress_bits(v):
    """Keep the even bits of v (uint64) and pack them into the low half."""
    v = v & np.uint64(0x5555555555555555)
    v = (v | (v >> np.uint64(1))) & np.uint64(0x3333333333333333)
    v = (v | (v >> np.uint64(2))) & np.uint64(0x0F0F0F0F0F0F0F0F)
    v = (v | (v >> np.uint64(4))) & np.uint64(0x00FF00FF00FF00FF)
    v = (v | (v >> np.uint64(8))) & np.uint64(0x0000FFFF0000FFFF)
    v = (v | (v >> np.uint64(16))) & np.uint64(0x00000000FFFFFFFF)
    return v


def _spread_bits(v):
    """Inverse of _compress_bits: put bit i of v at bit 2i."""
    v = v & np.uint64(0x00000000FFFFFFFF)
    v = (v | (v << np.uint64(16))) & np.uint64(0x0000FFFF0000FFFF)
    v = (v | (v << np.uint64(8))) & np.uint64(0x00FF00FF00FF00FF)
    v = (v | (v << np.uint64(4))) & np.uint64(0x0F0F0F0F0F0F0F0F)
    v = (v | (v << np.uint64(2))) & np.uint64(0x3333333333333333)
    v = (v | (v << np.uint64(1))) & np.uint64(0x5555555555555555)
    return v


def nest2xyf(nside, pix):
    """NEST index -> (ix, iy, face); NEST index = face*nside^2 + morton(ix, iy)."""
    pix = np.asarray(pix, dtype=np.int64)
    npface = int(nside) * int(nside)
    face = pix // npface
    p = (pix % npface).astype(np.uint64)
    ix = _compress_bits(p).astype(np.int64)
    iy = _compress_bits(p >> np.uint64(1)).astype(np.int64)
    return ix, iy, face


def xyf2nest(nside, ix, iy, face):
    ix = np.asarray(ix, dtype=np.int64).astype(np.uint64)
    iy = np.asarray(iy, dtype=np.int64).astype(np.uint64)
    m = _spread_bits(ix) | (_spread_bits(iy) << np.uint64(1))
    return np.asarray(face, dtype=np.int64) * (int(nside) * int(nside)) + m.astype(np.int64)


def _check_nside(nside):
    nside = int(nside)
    if not isnsideok(nside):
        raise ValueError(f"nside = {nside} is not a power of two >= 1")
    return nside


def nest2ring(nside, pix):
    """NEST index -> RING index (int64, pixelwise): ring ``jr`` and position ``jp`` in it from (face, ix, iy), the arithmetic
    of ``pix2vec``; rings are numbered from the north pole, the pixels of a ring by increasing phi."""
    nside = _check_nside(nside)
    ix, iy, face = nest2xyf(nside, pix)
    nl4 = 4 * nside
    jr = _JRLL[face] * nside - ix - iy - 1
    north = jr < nside
    south = jr > 3 * nside
    nr = np.where(north, jr, np.where(south, nl4 - jr, nside))
    before = np.where(north, 2 * nr * (nr - 1),
                      np.where(south, 12 * nside * nside - 2 * (nr + 1) * nr, 2 * nside * (nside - 1) + (jr - nside) * nl4))
    kshift = np.where(north | south, 0, (jr - nside) & 1)
    jp = (_JPLL[face] * nr + ix - iy + 1 + kshift) // 2
    jp = np.where(jp > nl4, jp - nl4, jp)
    jp = np.where(jp < 1, jp + nl4, jp)
    return before + jp - 1


def _isqrt(v):
    """floor(sqrt(v)) of non-negative int64, exact: the float64 root corrected by one either way."""
    v = np.asarray(v, dtype=np.int64)
    r = np.sqrt(v.astype(np.float64)).astype(np.int64)
    r = np.where(r * r > v, r - 1, r)
    return np.where((r + 1) * (r + 1) <= v, r + 1, r)


def ring2nest(nside, pix):
    """RING index -> NEST index (int64, pixelwise); the inverse of ``nest2ring``."""
    nside = _check_nside(nside)
    pix = np.asarray(pix, dtype=np.int64)
    npix = 12 * nside * nside
    ncap = 2 * nside * (nside - 1)
    nl4 = 4 * nside
    north = pix < ncap
    south = pix >= npix - ncap
    belt = ~(north | south)
    # caps: ring i (counted from the nearer pole) starts 2 i (i - 1) pixels from it and holds 4 i
    ip_n = np.where(north, pix, 0)
    ip_s = np.where(south, npix - pix, 1)  # 1 .. ncap from the south pole
    i_n = (1 + _isqrt(1 + 2 * ip_n)) >> 1
    i_s = (1 + _isqrt(2 * ip_s - 1)) >> 1
    ip_b = np.where(belt, pix - ncap, 0)
    i_b = ip_b // nl4 + nside
    iring = np.where(north, i_n, np.where(south, nl4 - i_s, i_b))  # ring number from the north pole, 1 .. 4 nside - 1
    nr = np.where(north, i_n, np.where(south, i_s, nside))
    iphi = np.where(north, ip_n + 1 - 2 * i_n * (i_n - 1),
                    np.where(south, 4 * i_s + 1 - (ip_s - 2 * i_s * (i_s - 1)), ip_b % nl4 + 1))
    kshift = np.where(belt, (iring + nside) & 1, 0)
    # the face: in the caps the quarter of the ring; in the belt from the two diagonals through the pixel
    ire = iring - nside + 1
    irm = 2 * nside + 2 - ire
    ifm = (iphi - ire // 2 + nside - 1) // nside
    ifp = (iphi - irm // 2 + nside - 1) // nside
    face_b = np.where(ifp == ifm, ifp | 4, np.where(ifp < ifm, ifp, ifm + 8))
    face = np.where(north, (iphi - 1) // nr, np.where(south, 8 + (iphi - 1) // nr, face_b))
    irt = iring - _JRLL[face] * nside + 1
    ipt = 2 * iphi - _JPLL[face] * nr - kshift - 1
    ipt = np.where(ipt >= 2 * nside, ipt - 8 * nside, ipt)
    ix = (ipt - irt) >> 1
    iy = (-ipt - irt) >> 1
    return xyf2nest(nside, ix, iy, face)


def reorder(m, r2n=False, n2r=False, axis=0):
    """A full-sky map (numpy, any dtype) in the other pixel ordering along ``axis``, like ``hp.reorder``: ``r2n`` RING -> NEST,
    ``n2r`` NEST -> RING; exactly one of them."""
    if bool(r2n) == bool(n2r):
        raise ValueError("reorder: set exactly one of r2n and n2r")
    m = np.asarray(m)
    npix = m.shape[axis]
    nside = npix2nside(npix)  # ValueError for a length that is not 12 nside^2
    _check_nside(nside)
    ids = np.arange(npix, dtype=np.int64)
    src = ring2nest(nside, ids) if n2r else nest2ring(nside, ids)  # out[i] = m[src[i]]
    return np.take(m, src, axis=axis)


def reorder_table(nside, indices, r2n=True):
    """The row permutation that reorders a partial-sky map: -> (perm int32, indices_ring int64).

    ``indices``: sorted unique NEST ids, the argument of ``HealpyGCNN``.  A RING-ordered map of the set holds its pixels sorted by
    RING id (``indices_ring``), a NEST-ordered one in the order of ``indices``.  ``r2n``: out[i] = in[perm[i]] takes RING rows to
    NEST rows; with ``r2n=False`` perm is the inverse (NEST rows to RING rows)."""
    nside = _check_nside(nside)
    indices = np.asarray(indices, dtype=np.int64).reshape(-1)
    if indices.size > 1 and not np.all(np.diff(indices) > 0):
        raise ValueError("indices must be sorted unique NEST ids")
    if indices.size and (indices[0] < 0 or indices[-1] >= nside2npix(nside)):
        raise ValueError(f"indices outside [0, {nside2npix(nside)})")
    ring = nest2ring(nside, indices)
    order = np.argsort(ring, kind="stable")  # RING row j is NEST row order[j]
    if r2n:
        perm = np.empty(indices.size, dtype=np.int64)
        perm[order] = np.arange(indices.size, dtype=np.int64)
    else:
        perm = order
    return perm.astype(np.int32), ring[order]


def pix2vec(nside, pix=None, dtype=np.float64):
    """Unit vectors of NEST pixel centres, shape (len(pix), 3)."""
    nside = int(nside)
    if pix is None:
        pix = np.arange(nside2npix(nside), dtype=np.int64)
    ix, iy, face = nest2xyf(nside, pix)
    nl4 = 4 * nside
    npix = 12 * nside * nside
    fact2 = 4.0 / npix
    fact1 = (2 * nside) * fact2
    jr = _JRLL[face] * nside - ix - iy - 1
    north = jr < nside
    south = jr > 3 * nside
    belt = ~(north | south)
    nr = np.where(north, jr, np.where(south, nl4 - jr, nside))
    z = np.empty(jr.shape, dtype=np.float64)
    z[north] = 1.0 - (nr[north].astype(np.float64) ** 2) * fact2
    z[south] = (nr[south].astype(np.float64) ** 2) * fact2 - 1.0
    z[belt] = (2 * nside - jr[belt]) * fact1
    kshift = np.where(belt, (jr - nside) & 1, 0)
    jp = (_JPLL[face] * nr + ix - iy + 1 + kshift) // 2
    jp = np.where(jp > nl4, jp - nl4, jp)
    jp = np.where(jp < 1, jp + nl4, jp)
    phi = (jp - (kshift + 1) * 0.5) * ((np.pi / 2) / nr)
    st = np.sqrt(np.maximum(0.0, (1.0 - z) * (1.0 + z)))
    out = np.empty(jr.shape + (3,), dtype=dtype)
    out[..., 0] = st * np.cos(phi)
    out[..., 1] = st * np.sin(phi)
    out[..., 2] = z
    return out


def neighbours(nside, pix=None):
    """The 8 grid neighbours (SW, W, NW, N, NE, E, SE, S) of NEST pixels; -1 where absent.

    Every pixel has 8 of them except the 24 pixels at the 8 corners where only three
    faces meet, which have 7.
    """
    nside = int(nside)
    if pix is None:
        pix = np.arange(nside2npix(nside), dtype=np.int64)
    pix = np.asarray(pix, dtype=np.int64)
    ix, iy, face = nest2xyf(nside, pix)
    out = np.empty(pix.shape + (8,), dtype=np.int64)
    for i in range(8):
        x = ix + _NB_XOFF[i]
        y = iy + _NB_YOFF[i]
        nb = np.full(pix.shape, 4, dtype=np.int64)
        lo = x < 0
        hi = x >= nside
        x = np.where(lo, x + nside, np.where(hi, x - nside, x))
        nb = nb - lo + hi
        lo = y < 0
        hi = y >= nside
        y = np.where(lo, y + nside, np.where(hi, y - nside, y))
        nb = nb - 3 * lo + 3 * hi
        f = _NB_FACE[nb, face]
        bits = _NB_SWAP[nb, face >> 2]
        x = np.where(bits & 1, nside - x - 1, x)
        y = np.where(bits & 2, nside - y - 1, y)
        sw = (bits & 4) != 0
        x, y = np.where(sw, y, x), np.where(sw, x, y)
        res = xyf2nest(nside, x, y, np.maximum(f, 0))
        out[..., i] = np.where(f >= 0, res, -1)
    return out


# Gaussian kernel widths of the reference's graph producer for k = 8 and 20 neighbours
# (recalled from the pygsp fork, unverifiable here; other values are
# extrapolated ~ c_k / nside).  Treated as a parameter: the convolution takes L as input.
_KW_TABLE = {
    8: {32: 0.02500, 64: 0.01228, 128: 0.00614, 256: 0.00307, 512: 0.00154, 1024: 0.00077},
    20: {32: 0.03185, 64: 0.01564, 128: 0.00782, 256: 0.00391, 512: 0.00196, 1024: 0.00098},
}
_KW_COEFF = {8: 0.786, 20: 1.001, 40: 1.3, 60: 1.55}


def kernel_width(nside, n_neighbors=8):
    tab = _KW_TABLE.get(int(n_neighbors), {})
    if int(nside) in tab:
        return tab[int(nside)]
    return _KW_COEFF.get(int(n_neighbors), 0.786 * np.sqrt(n_neighbors / 8.0)) / float(nside)


def _normalized_laplacian(W):
    d = np.asarray(W.sum(axis=1)).ravel()
    with np.errstate(divide="ignore"):
        dis = np.where(d > 0, 1.0 / np.sqrt(d), 0.0)
    D = sparse.diags(dis)
    M = W.shape[0]
    return (sparse.identity(M, format="csr", dtype=np.float64) - D @ W @ D).tocsr()


def healpix_graph(nside, indices=None, n_neighbors=8, mode="knn", kw=None):
    """Weighted adjacency W (CSR, float64, symmetric, zero diagonal) on NEST pixels.

    mode="knn":  symmetrised k-nearest-neighbour graph on the 3-D pixel centres with weights
                 exp(-(d/kw)^2) -- the family ``SphereHealpix(k=n_neighbors)`` produces
                 (``healpy_networks.py:110-118``); rows end up with k..k+2 neighbours.
    mode="grid": the fixed 8-neighbour HEALPix stencil (7 at the 24 corner pixels) with the
                 same kernel; cheap enough for nside >= 1024.
    ``indices``: sorted NEST pixel ids of a partial-sky map; the graph is built on that subset
                 only, like the reference passing ``indexes=current_indices``.
    """
    nside = int(nside)
    npix = nside2npix(nside)
    if indices is None:
        indices = np.arange(npix, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    M = indices.shape[0]
    if kw is None:
        kw = kernel_width(nside, n_neighbors)
    vec = pix2vec(nside, indices)
    if mode == "knn":
        from scipy.spatial import cKDTree

        k = int(n_neighbors)
        tree = cKDTree(vec)
        dist, nbr = tree.query(vec, k=k + 1)
        rows = np.repeat(np.arange(M, dtype=np.int64), k)
        cols = nbr[:, 1:].reshape(-1).astype(np.int64)
        w = np.exp(-((dist[:, 1:].reshape(-1) / kw) ** 2))
        A = sparse.csr_matrix((w, (rows, cols)), shape=(M, M))
        # symmetrise: an edge present in one direction is filled in the other
        W = A.maximum(A.T).tocsr()
    elif mode == "grid":
        if int(n_neighbors) != 8:
            raise NotImplementedError("the grid stencil has 8 neighbours")
        nb = neighbours(nside, indices)
        full = M == npix
        if not full:
            lut = np.full(npix, -1, dtype=np.int64)
            lut[indices] = np.arange(M, dtype=np.int64)
            nb = np.where(nb >= 0, lut[np.maximum(nb, 0)], -1)
        rows = np.repeat(np.arange(M, dtype=np.int64), 8)
        cols = nb.reshape(-1)
        ok = cols >= 0
        rows, cols = rows[ok], cols[ok]
        d = np.linalg.norm(vec[rows] - vec[cols], axis=1)
        w = np.exp(-((d / kw) ** 2))
        W = sparse.csr_matrix((w, (rows, cols)), shape=(M, M))
        W = W.maximum(W.T).tocsr()
    else:
        raise ValueError(f"unknown graph mode <{mode}>")
    W.setdiag(0.0)
    W.eliminate_zeros()
    W.sort_indices()
    return W


def healpix_laplacian(nside, indices=None, n_neighbors=8, mode="knn", kw=None):
    """Normalised Laplacian L = I - D^-1/2 W D^-1/2 (CSR float64) of ``healpix_graph``."""
    return _normalized_laplacian(healpix_graph(nside, indices, n_neighbors, mode, kw))


def grid_laplacian_ell(nside, kw=None, dtype=np.float64, chunk=1 << 22):
    """Full-sphere 8-neighbour normalised Laplacian directly in padded-ELL form.

    Returns (cols int32 [M,9], vals dtype [M,9]); slot 0 is the diagonal (1.0), slots 1..8
    the grid neighbours in ``neighbours`` order, absent ones padded with (col=row, val=0).
    Same matrix as ``healpix_laplacian(nside, mode="grid")`` without the scipy round trip,
    which at nside 1024 (12.6 M rows) costs minutes.
    """
    nside = int(nside)
    npix = nside2npix(nside)
    if kw is None:
        kw = kernel_width(nside, 8)
    cols = np.empty((npix, 9), dtype=np.int32)
    w = np.empty((npix, 9), dtype=np.float64)
    for s in range(0, npix, chunk):
        e = min(npix, s + chunk)
        p = np.arange(s, e, dtype=np.int64)
        nb = neighbours(nside, p)
        v0 = pix2vec(nside, p)
        cols[s:e, 0] = p
        w[s:e, 0] = 0.0
        for j in range(8):
            ok = nb[:, j] >= 0
            q = np.where(ok, nb[:, j], p)
            d = np.linalg.norm(pix2vec(nside, q) - v0, axis=1)
            cols[s:e, j + 1] = q
            w[s:e, j + 1] = np.where(ok, np.exp(-((d / kw) ** 2)), 0.0)
    deg = w.sum(axis=1)
    dis = 1.0 / np.sqrt(deg)
    vals = np.empty((npix, 9), dtype=dtype)
    for s in range(0, npix, chunk):
        e = min(npix, s + chunk)
        vals[s:e] = (-(w[s:e] * dis[s:e, None]) * dis[cols[s:e]]).astype(dtype)
        vals[s:e, 0] = 1.0
    return cols, vals


def cap_indices(nside, vec=(1.0, 0.0, 0.0), fraction=1.0 / 3.0):
    """Sorted NEST ids of the spherical cap around ``vec`` covering ``fraction`` of the sphere."""
    v = np.asarray(vec, dtype=np.float64)
    v = v / np.linalg.norm(v)
    cos_lim = 1.0 - 2.0 * float(fraction)
    c = pix2vec(int(nside)) @ v
    return np.nonzero(c >= cos_lim)[0].astype(np.int64)


def extend_indices(indices, nside_in, nside_out, nest=True):
    """Minimal superset of ``indices`` that coarsens cleanly to ``nside_out``.

    Same contract as the reference's ``utils.extend_indices`` (``utils.py:9-37``, which
    degrades and re-upgrades a 0/1 map with healpy): in NEST order a pixel's parent at
    nside_out is ``pix >> 2*log2(nside_in/nside_out)``, so the answer is every child of
    every touched parent.  With ``nest=False`` the ids are RING ids on both sides (sorted on the way out): through
    ``ring2nest``, the NEST rule and ``nest2ring``.
    """
    if not nest:
        return np.sort(nest2ring(nside_in, extend_indices(ring2nest(nside_in, indices), nside_in, nside_out, nest=True)))
    indices = np.asarray(indices, dtype=np.int64)
    ratio = int(nside_in) // int(nside_out)
    if ratio < 1 or ratio * int(nside_out) != int(nside_in) or not isnsideok(ratio):
        raise ValueError("nside_in must be nside_out times a power of two")
    per = ratio * ratio
    parents = np.unique(indices // per)
    return (parents[:, None] * per + np.arange(per, dtype=np.int64)[None, :]).reshape(-1)


def superpixel_padding_mask(indices, footprint, p):
    """The key mask of ``Healpy_ViT(p, ..., mask=...)`` for a padded survey footprint: 1.0 for every super-pixel that holds
    nothing but padding.

    :param indices: the sorted NEST ids the network runs on -- closed under ``p`` coarsenings (every touched parent ``id >> 2 p``
        has all its 4^p children in the set, what ``extend_indices`` returns); anything else raises ValueError
    :param footprint: the NEST ids (same nside) that hold data
    :param p: the super-pixel size factor of the ViT layer: a super-pixel is the 4^p children of a pixel p levels coarser
    :return: float32 (len(indices) / 4^p,), in the order of the coarsened index set (ascending parent id, the order of the
        layer's tokens): 1.0 where the super-pixel contains no footprint pixel ("do not attend"), 0.0 elsewhere -- one data pixel
        keeps a super-pixel attended
    """
    indices = np.asarray(indices, dtype=np.int64).reshape(-1)
    per = 4 ** int(p)
    if int(p) < 1:
        raise ValueError("p has to be at least 1")
    if indices.size % per != 0 or (indices.size > 1 and not np.all(np.diff(indices) > 0)):
        raise ValueError(f"indices must be sorted NEST ids closed under p = {p} coarsenings ({indices.size} ids, patches of {per})")
    blocks = indices.reshape(-1, per)
    parents = blocks[:, 0] // per
    if not np.array_equal(blocks, parents[:, None] * per + np.arange(per, dtype=np.int64)[None, :]):
        raise ValueError(f"indices are not closed under p = {p} coarsenings: a parent pixel lacks some of its {per} children "
                         "(healpix.extend_indices pads a footprint to such a set)")
    touched = np.unique(np.asarray(footprint, dtype=np.int64).reshape(-1) // per)
    return (~np.isin(parents, touched)).astype(np.float32)


# ----------------------------------------------------------------------------------------------
# torch twin of the grid-stencil builder: same algorithm on torch tensors, so that a 12.6 M-pixel
# (nside 1024) Laplacian is produced in well under a second on the GPU instead of minutes in numpy.
# Checked against the numpy functions above in tests/test_host.py.
# ----------------------------------------------------------------------------------------------


def _t_compress(v):
    v = v & 0x5555555555555555
    v = (v | (v >> 1)) & 0x3333333333333333
    v = (v | (v >> 2)) & 0x0F0F0F0F0F0F0F0F
    v = (v | (v >> 4)) & 0x00FF00FF00FF00FF
    v = (v | (v >> 8)) & 0x0000FFFF0000FFFF
    v = (v | (v >> 16)) & 0x00000000FFFFFFFF
    return v


def _t_spread(v):
    v = v & 0x00000000FFFFFFFF
    v = (v | (v << 16)) & 0x0000FFFF0000FFFF
    v = (v | (v << 8)) & 0x00FF00FF00FF00FF
    v = (v | (v << 4)) & 0x0F0F0F0F0F0F0F0F
    v = (v | (v << 2)) & 0x3333333333333333
    v = (v | (v << 1)) & 0x5555555555555555
    return v


def _t_pix2vec(nside, ix, iy, face, jrll, jpll):
    import torch

    nl4 = 4 * nside
    fact2 = 4.0 / (12 * nside * nside)
    fact1 = (2 * nside) * fact2
    jr = jrll[face] * nside - ix - iy - 1
    north = jr < nside
    south = jr > 3 * nside
    belt = ~(north | south)
    nr = torch.where(north, jr, torch.where(south, nl4 - jr, torch.full_like(jr, nside)))
    nrf = nr.to(torch.float64)
    z = torch.where(north, 1.0 - nrf * nrf * fact2,
                    torch.where(south, nrf * nrf * fact2 - 1.0, (2 * nside - jr).to(torch.float64) * fact1))
    kshift = torch.where(belt, (jr - nside) & 1, torch.zeros_like(jr))
    jp = torch.div(jpll[face] * nr + ix - iy + 1 + kshift, 2, rounding_mode="floor")
    jp = torch.where(jp > nl4, jp - nl4, jp)
    jp = torch.where(jp < 1, jp + nl4, jp)
    phi = (jp.to(torch.float64) - (kshift + 1).to(torch.float64) * 0.5) * ((np.pi / 2) / nrf)
    st = torch.sqrt(torch.clamp((1.0 - z) * (1.0 + z), min=0.0))
    return torch.stack((st * torch.cos(phi), st * torch.sin(phi), z), dim=-1)


class _GridTables:
    """The face tables of ``neighbours`` as tensors on one device."""

    def __init__(self, dev):
        import torch

        self.jrll = torch.as_tensor(_JRLL, device=dev)
        self.jpll = torch.as_tensor(_JPLL, device=dev)
        self.nbface = torch.as_tensor(_NB_FACE, device=dev)
        self.nbswap = torch.as_tensor(_NB_SWAP, device=dev)


def _t_grid_pixels(nside, p, tab):
    """(ix, iy, face, unit vectors) of the NEST pixels ``p`` (int64 tensor)."""
    import torch

    npface = nside * nside
    face = torch.div(p, npface, rounding_mode="floor")
    pm = p - face * npface
    ix = _t_compress(pm)
    iy = _t_compress(pm >> 1)
    return ix, iy, face, _t_pix2vec(nside, ix, iy, face, tab.jrll, tab.jpll)


def _t_grid_neighbour(nside, kw, p, ix, iy, face, v0, i, tab):
    """Grid neighbour ``i`` (the direction order of ``neighbours``) of the pixels ``p``: -> (ok, q, w) -- whether it exists, its
    NEST id (``p`` itself where it does not) and the kernel weight exp(-(d / kw)^2) (0 where it does not)."""
    import torch

    npface = nside * nside
    x = ix + int(_NB_XOFF[i])
    y = iy + int(_NB_YOFF[i])
    lo, hi = x < 0, x >= nside
    x = torch.where(lo, x + nside, torch.where(hi, x - nside, x))
    nb = 4 - lo.to(torch.int64) + hi.to(torch.int64)
    lo, hi = y < 0, y >= nside
    y = torch.where(lo, y + nside, torch.where(hi, y - nside, y))
    nb = nb - 3 * lo.to(torch.int64) + 3 * hi.to(torch.int64)
    f = tab.nbface[nb, face]
    bits = tab.nbswap[nb, face >> 2]
    x = torch.where((bits & 1) != 0, nside - x - 1, x)
    y = torch.where((bits & 2) != 0, nside - y - 1, y)
    sw = (bits & 4) != 0
    x, y = torch.where(sw, y, x), torch.where(sw, x, y)
    ok = f >= 0
    fq = torch.clamp(f, min=0)
    q = torch.where(ok, fq * npface + (_t_spread(x) | (_t_spread(y) << 1)), p)
    d = torch.linalg.norm(_t_pix2vec(nside, x, y, fq, tab.jrll, tab.jpll) - v0, dim=1)
    return ok, q, torch.where(ok, torch.exp(-((d / kw) ** 2)), torch.zeros_like(d))


def grid_laplacian_ell_torch(nside, kw=None, device="cpu", chunk=1 << 22):
    """``grid_laplacian_ell`` on torch tensors: (cols int32 [M,9], vals float64 [M,9]) on ``device``."""
    import torch

    nside = int(nside)
    npix = 12 * nside * nside
    if kw is None:
        kw = kernel_width(nside, 8)
    dev = torch.device(device)
    tab = _GridTables(dev)
    cols = torch.empty((npix, 9), dtype=torch.int32, device=dev)
    w = torch.zeros((npix, 9), dtype=torch.float64, device=dev)
    for s in range(0, npix, chunk):
        e = min(npix, s + chunk)
        p = torch.arange(s, e, dtype=torch.int64, device=dev)
        ix, iy, face, v0 = _t_grid_pixels(nside, p, tab)
        cols[s:e, 0] = p.to(torch.int32)
        for i in range(8):
            _, q, wi = _t_grid_neighbour(nside, kw, p, ix, iy, face, v0, i, tab)
            cols[s:e, i + 1] = q.to(torch.int32)
            w[s:e, i + 1] = wi
    dis = 1.0 / torch.sqrt(w.sum(dim=1))
    vals = -(w * dis[:, None]) * dis[cols.to(torch.int64)]
    vals[:, 0] = 1.0
    return cols, vals


# ----------------------------------------------------------------------------------------------
# Graphs built on the device: the k nearest pixels from the HIP kernel (csrc/healpix_knn.hip), everything
# between them and the padded-ELL Laplacian as torch operators on the same device.  What HealpyGCNN(build="device")
# runs in place of healpix_graph / healpix_laplacian / utils.csr_to_ell.
# ----------------------------------------------------------------------------------------------


def _index_set(nside, indices):
    """``indices`` as a checked int64 array of sorted unique NEST ids, or None for the full sky (also a set that is all of it)."""
    nside = _check_nside(nside)
    npix = nside2npix(nside)
    if indices is None:
        return None
    ind = np.ascontiguousarray(np.asarray(indices).reshape(-1), dtype=np.int64)
    if ind.size > 1 and not np.all(np.diff(ind) > 0):
        raise ValueError("indices must be sorted unique NEST ids")
    if ind.size and (ind[0] < 0 or ind[-1] >= npix):
        raise ValueError(f"indices outside [0, {npix})")
    return None if ind.size == npix else ind


def _device_lut(nside, ind, dev):
    """(indices int64 [M], lut int32 [npix]: NEST id -> row of the set or -1) on ``dev``."""
    import torch

    ti = torch.as_tensor(ind, device=dev)
    lut = torch.full((nside2npix(nside),), -1, dtype=torch.int32, device=dev)
    lut[ti] = torch.arange(ti.shape[0], dtype=torch.int32, device=dev)
    return ti, lut


def healpix_knn_device(nside, indices=None, n_neighbors=8, device="cuda"):
    """The ``n_neighbors`` nearest pixels of every pixel of the set, on the device: -> (nbr int32 [M, k], d2 float64 [M, k],
    completed) -- rows of the set and squared chords, every row ascending by distance; ``completed``: how many rows the kernel
    flagged (``_native.healpix_knn``: its window could not guarantee them -- the edge of a footprint) and a ``cKDTree`` over the
    set's vectors filled in on the host, those rows only.

    At the k-th neighbour HEALPix has exact ties (mirror pairs of pixels); which member of a tied pair a row holds is not
    specified, and need not be the one ``healpix_graph(mode="knn")`` picks."""
    import torch

    from . import _native

    nside, k = _check_nside(nside), int(n_neighbors)
    ind = _index_set(nside, indices)
    dev = torch.device(device)
    if ind is None:
        nbr, d2, ok = _native.healpix_knn(nside, k, device=dev)
    else:
        nbr, d2, ok = _native.healpix_knn(nside, k, *_device_lut(nside, ind, dev))
    bad = torch.nonzero(ok == 0).reshape(-1)
    if bad.numel():
        from scipy.spatial import cKDTree

        rows = bad.cpu().numpy()
        vec = pix2vec(nside, ind)
        _, nb = cKDTree(vec).query(vec[rows], k=k + 1)
        nb = nb.reshape(rows.shape[0], k + 1)
        # the row itself (distance 0) is among the k + 1: to the end; the others by (d2, row), as the kernel orders a row
        order = np.argsort(nb == rows[:, None], axis=1, kind="stable")
        nb = np.take_along_axis(nb, order, axis=1)[:, :k]
        dd = ((vec[nb] - vec[rows][:, None, :]) ** 2).sum(axis=2)
        order = np.lexsort((nb, dd), axis=1)
        nb, dd = np.take_along_axis(nb, order, axis=1), np.take_along_axis(dd, order, axis=1)
        nbr[bad] = torch.as_tensor(nb.astype(np.int32), device=nbr.device)
        d2[bad] = torch.as_tensor(dd, device=d2.device)
    return nbr, d2, int(bad.numel())


class DeviceGraph:
    """The symmetrised weighted graph of ``healpix_graph`` as sorted coordinate lists on a device: ``rows``, ``cols`` (int64) and
    ``w`` (float64), ascending by (row, col), zero diagonal, no zero weights.  ``M``: number of pixels; ``completed``: rows of
    the k-NN search that were completed on the host."""

    def __init__(self, M, rows, cols, w, completed=0):
        self.M, self.rows, self.cols, self.w, self.completed = int(M), rows, cols, w, int(completed)

    @property
    def nnz(self):
        return int(self.rows.shape[0])

    def _table(self, rows, cols, vals, pad_col, pad_val):
        """Entries sorted by (row, col) as a padded table [M, W], W = the longest row (at least 1): -> (cols int32, vals)."""
        import torch

        dev, M = rows.device, self.M
        lens = torch.bincount(rows, minlength=M)
        W = max(int(lens.max()) if rows.numel() else 0, 1)
        slot = torch.arange(rows.shape[0], dtype=torch.int64, device=dev) - (torch.cumsum(lens, 0) - lens)[rows]
        if pad_col is None:  # the row itself
            tc = torch.arange(M, dtype=torch.int32, device=dev)[:, None].repeat(1, W)
        else:
            tc = torch.full((M, W), pad_col, dtype=torch.int32, device=dev)
        tc[rows, slot] = cols.to(torch.int32)
        tv = None
        if vals is not None:
            tv = torch.full((M, W), pad_val, dtype=vals.dtype, device=dev)
            tv[rows, slot] = vals
        return tc, tv

    def adjacency_table(self):
        """The neighbour table ``utils.adjacency_to_ell`` gives for this graph: int32 [M, W], the columns of a row ascending,
        then -1."""
        return self._table(self.rows, self.cols, None, -1, None)[0]

    def laplacian_ell(self):
        """I - D^-1/2 W D^-1/2 in the layout of ``utils.csr_to_ell``: (cols int32 [M, W], vals float64 [M, W]), the columns of a
        row ascending with the diagonal where it falls among them, padding (col = row, val = 0)."""
        import torch

        dev, M = self.rows.device, self.M
        diag = torch.arange(M, dtype=torch.int64, device=dev)
        key, order = torch.sort(torch.cat((self.rows * M + self.cols, diag * (M + 1))))
        w = torch.cat((self.w, torch.full((M,), -1.0, dtype=torch.float64, device=dev)))[order]  # (-1: marks the diagonal)
        rows = torch.div(key, M, rounding_mode="floor")
        cols, w = self._table(rows, key - rows * M, w, None, 0.0)
        del key, order, rows
        on_diag = w < 0
        w = torch.where(on_diag, torch.zeros_like(w), w)
        deg = w.sum(dim=1)  # (along a row of the table: a fixed order, unlike an atomic scatter)
        dis = torch.where(deg > 0, 1.0 / torch.sqrt(deg), torch.zeros_like(deg))
        vals = 0.0 - (dis[:, None] * w) * dis[cols.to(torch.int64)]  # (D W) D as the host multiplies; 0 - x: padding stays +0
        vals[on_diag] = 1.0
        return cols, vals


def _symmetrise(M, rows, cols, w):
    """max(A, A^T) of coordinate entries on a device, without its zeros: -> sorted unique (rows, cols, w)."""
    import torch

    key, order = torch.sort(torch.cat((rows * M + cols, cols * M + rows)))
    w = torch.cat((w, w))[order]
    del order
    key, inv = torch.unique_consecutive(key, return_inverse=True)
    w = torch.zeros(key.shape, dtype=w.dtype, device=w.device).scatter_reduce_(0, inv, w, "amax", include_self=False)
    del inv
    keep = w != 0  # (eliminate_zeros of the host: a weight that underflowed is no edge)
    key, w = key[keep], w[keep]
    r = torch.div(key, M, rounding_mode="floor")
    return r, key - r * M, w


def healpix_graph_device(nside, indices=None, n_neighbors=8, mode="knn", kw=None, device="cuda"):
    """``healpix_graph`` built on the device: -> ``DeviceGraph``.  mode="knn": neighbours from the HIP kernel
    (``healpix_knn_device``: ties at the k-th neighbour may be broken differently from the host's k-d tree); mode="grid": the
    8-neighbour stencil, neighbours outside the set dropped.  Weights exp(-(d / kw)^2), max(A, A^T), zero diagonal, as the host."""
    import torch

    nside = _check_nside(nside)
    ind = _index_set(nside, indices)
    dev = torch.device(device)
    if kw is None:
        kw = kernel_width(nside, n_neighbors)
    M = nside2npix(nside) if ind is None else int(ind.shape[0])
    completed = 0
    if mode == "knn":
        k = int(n_neighbors)
        nbr, d2, completed = healpix_knn_device(nside, ind, k, dev)
        rows = torch.arange(M, dtype=torch.int64, device=dev).repeat_interleave(k)
        cols = nbr.reshape(-1).to(torch.int64)
        w = torch.exp(-((torch.sqrt(d2.reshape(-1)) / kw) ** 2))
        del nbr, d2
    elif mode == "grid":
        if int(n_neighbors) != 8:
            raise NotImplementedError("the grid stencil has 8 neighbours")
        tab = _GridTables(dev)
        if ind is None:
            p, lut = torch.arange(M, dtype=torch.int64, device=dev), None
        else:
            p, lut = _device_lut(nside, ind, dev)
        ix, iy, face, v0 = _t_grid_pixels(nside, p, tab)
        rr, cc, ww = [], [], []
        own = torch.arange(M, dtype=torch.int64, device=dev)
        for i in range(8):
            ok, q, wi = _t_grid_neighbour(nside, kw, p, ix, iy, face, v0, i, tab)
            if lut is not None:
                q = lut[q].to(torch.int64)
                ok = ok & (q >= 0)
            rr.append(own[ok]); cc.append(q[ok]); ww.append(wi[ok])
        rows, cols, w = torch.cat(rr), torch.cat(cc), torch.cat(ww)
    else:
        raise ValueError(f"unknown graph mode <{mode}>")
    return DeviceGraph(M, *_symmetrise(M, rows, cols, w), completed=completed)


def healpix_laplacian_ell(nside, indices=None, n_neighbors=8, mode="knn", kw=None, device="cuda"):
    """The matrix ``healpix_laplacian`` defines, built on the device and already in the padded-ELL layout of
    ``utils.csr_to_ell``: -> (cols int32 [M, W], vals float64 [M, W]) torch tensors on ``device``; the columns of a row ascend, the
    diagonal sits where it falls in that order, padding is (col = row, val = 0) -- so a layer over this table sums a row in the
    order a layer over the host's matrix does.

    mode="knn": ``healpix_graph_device`` (the HIP k-NN kernel; rows it flags are completed on the host).  Not bit-identical to
    the host's matrix where the k-th neighbour is tied: either member of a tied pair is a correct k-NN graph.
    mode="grid": the full sky from ``grid_laplacian_ell_torch``, brought into the layout above; a partial sky with the neighbours
    outside the set dropped and the degrees taken over what remains, as the host does."""
    import torch

    nside = _check_nside(nside)
    ind = _index_set(nside, indices)
    if mode == "grid" and ind is None:
        if int(n_neighbors) != 8:
            raise NotImplementedError("the grid stencil has 8 neighbours")
        cols, vals = grid_laplacian_ell_torch(nside, kw=kw, device=device)
        M = cols.shape[0]
        pad = vals == 0  # (absent neighbours of the 24 corner pixels: col = row, val = 0)
        order = torch.argsort(torch.where(pad, torch.full_like(cols, M), cols), dim=1, stable=True)
        return torch.gather(cols, 1, order), torch.gather(vals, 1, order)
    return healpix_graph_device(nside, ind, n_neighbors, mode, kw, device).laplacian_ell()


def healpix_adjacency_tables(nside, indices=None, n_neighbors=8, mode="knn", kw=None, device="cuda", graph=None):
    """The neighbour tables of ``Healpy_Transformer`` for the graph of ``healpix_graph_device`` (or a ``DeviceGraph`` already
    built: ``graph``): -> (nbr, nbrT) int32 [M, W] on the device, what ``utils.adjacency_to_ell`` gives for the graph and for its
    transpose -- ONE tensor, the graph being symmetric."""
    if graph is None:
        graph = healpix_graph_device(nside, indices, n_neighbors, mode, kw, device)
    nbr = graph.adjacency_table()
    return nbr, nbr


# ----------------------------------------------------------------------------------------------
# The kernel table of HealpySmoothing built on the device (csrc/healpix_disc.hip): what HealpySmoothing(build="device")
# runs in place of its k-d tree, numpy sort and scipy transpose.
# ----------------------------------------------------------------------------------------------


def gauss_table_device(nside, indices, sigma_rad, n_sigma_support=3, device="cuda", want_raw=False):
    """The table of ``HealpySmoothing`` for the pixels ``indices`` (unique NEST ids in any order; rows follow that order), on
    the device: -> ``(cols int32 [M, W], vals float32 [M, W], raw float32 [M, W] or None, W, completed)``.

    W is the largest number of pixels of the set within ``min(n_sigma_support * sigma_rad, pi)`` of a pixel
    (``_native.healpix_disc_count``; rows it flags are counted by a ``cKDTree.query_ball_point``, those rows only).  A row holds
    the W nearest pixels of the set, columns ascending, Gaussian weights normalised to sum 1 (``_native.healpix_gauss_table``;
    rows it flags are completed on the host with the arithmetic of ``HealpySmoothing._build_tree`` / ``_finish_table``, those
    rows only, and written into the device tables).  ``raw``: the weights before normalisation, with ``want_raw``.
    ``completed``: the number of rows that needed the host in either kernel.

    At the W-th neighbour HEALPix has exact ties; which member of a tied pair a row holds is not specified and need not be the
    one the host-built layer picks."""
    import torch

    from . import _native

    nside = _check_nside(nside)
    npix = nside2npix(nside)
    ind = np.ascontiguousarray(np.asarray(indices).reshape(-1), dtype=np.int64)
    M = int(ind.shape[0])
    if M < 1 or ind.min() < 0 or ind.max() >= npix or np.unique(ind).shape[0] != M:
        raise ValueError(f"indices must be unique NEST ids in [0, {npix})")
    sigma_rad = float(sigma_rad)
    rho = min(sigma_rad * float(n_sigma_support), np.pi)
    if not (sigma_rad > 0.0 and rho > 0.0):
        raise ValueError("sigma_rad and n_sigma_support must be positive")
    chord = 2.0 * np.sin(0.5 * rho)
    dev = torch.device(device)
    full = M == npix and bool(np.all(ind == np.arange(npix)))
    pixel_set = (None, None) if full else _device_lut(nside, ind, dev)
    dev = dev if full else None  # (a set brings its device along)
    count, ok = _native.healpix_disc_count(nside, chord * chord, *pixel_set, device=dev)
    bad_count = torch.nonzero(ok == 0).reshape(-1).cpu().numpy()
    tree = vec = None
    if bad_count.size:
        from scipy.spatial import cKDTree

        vec = pix2vec(nside, ind)
        tree = cKDTree(vec)
        lens = tree.query_ball_point(vec[bad_count], chord, return_length=True)
        count[torch.as_tensor(bad_count, device=count.device)] = torch.as_tensor(np.asarray(lens, dtype=np.int32), device=count.device)
    W = int(count.max())
    if W > _native.DISC_MAX_W:
        raise ValueError(f"the smoothing kernel has rows of W = {W} entries; the device build takes up to {_native.DISC_MAX_W} "
                         f'(_native.DISC_MAX_W): build the layer with build="host"')
    cols, vals, raw, ok = _native.healpix_gauss_table(nside, W, sigma_rad, rho, *pixel_set, device=dev, want_raw=want_raw)
    bad = torch.nonzero(ok == 0).reshape(-1)
    if bad.numel():
        from scipy.spatial import cKDTree

        rows = bad.cpu().numpy()
        if tree is None:
            vec = pix2vec(nside, ind)
            tree = cKDTree(vec)
        dist, nb = tree.query(vec[rows], k=W)
        dist, nb = dist.reshape(-1, W), nb.reshape(-1, W)
        theta = 2.0 * np.arcsin(np.minimum(0.5 * dist, 1.0))
        v = np.exp(-0.5 / sigma_rad**2 * theta**2).astype(np.float32)  # (HealpySmoothing.kernel_func)
        order = np.argsort(nb, axis=1, kind="stable")
        nb, v = np.take_along_axis(nb, order, axis=1), np.take_along_axis(v, order, axis=1)
        cols[bad] = torch.as_tensor(nb.astype(np.int32), device=cols.device)
        vals[bad] = torch.as_tensor((v / v.sum(axis=1, dtype=np.float64, keepdims=True)).astype(np.float32), device=vals.device)
        if raw is not None:
            raw[bad] = torch.as_tensor(v, device=raw.device)
        completed = int(np.union1d(rows, bad_count).shape[0])
    else:
        completed = int(bad_count.shape[0])
    return cols, vals, raw, W, completed


def transpose_table(cols, vals):
    """The table of the transposed matrix in the layout of ``HealpySmoothing._transposed_tables``, with torch operators on the
    tensors' device: zero values dropped, the columns of a row ascending, every row padded to the longest with (column = the row
    itself, value = 0); -> (int32 [M, WT], float32 [M, WT]).  A permutation of the entries: no arithmetic on the values."""
    import torch

    M, W = cols.shape
    dev = cols.device
    c = cols.reshape(-1)
    v = vals.reshape(-1)
    r = torch.arange(M, dtype=torch.int32, device=dev).repeat_interleave(W)
    keep = v != 0
    if not bool(keep.all()):
        c, v, r = c[keep], v[keep], r[keep]
    # entries are filed by ascending row: a stable sort by column leaves the rows of a column ascending
    c, order = torch.sort(c.to(torch.int64), stable=True)
    v, r = v[order], r[order]
    del order
    lens = torch.bincount(c, minlength=M)
    WT = max(int(lens.max()) if c.numel() else 0, 1)
    slot = torch.arange(c.shape[0], dtype=torch.int64, device=dev) - (torch.cumsum(lens, 0) - lens)[c]
    colsT = torch.arange(M, dtype=torch.int32, device=dev)[:, None].repeat(1, WT)
    valsT = torch.zeros((M, WT), dtype=torch.float32, device=dev)
    colsT[c, slot] = r
    valsT[c, slot] = v.to(torch.float32)
    return colsT, valsT


# ----------------------------------------------------------------------------------------------
# From points to pixels: ang2pix / vec2pix / pix2ang and healpy's bilinear interpolation (get_interp_weights, get_interp_val),
# numpy float64, healpy's names and conventions.  The reference of the rotation kernel (csrc/healpix_interp.hip, whose stencil
# function is this arithmetic statement by statement) and what HealpyRotate runs on CPU tensors.
# ----------------------------------------------------------------------------------------------

_TWOPI = 2.0 * np.pi


def _reduce_phi(phi):
    """phi into [0, 2 pi]: a float64 phi of -1e-17 becomes exactly 2 pi (callers wrap ring positions, they do not assume < 2 pi)."""
    phi = np.fmod(np.asarray(phi, dtype=np.float64), _TWOPI)
    return np.where(phi < 0, phi + _TWOPI, phi)


def _ring_info(nside, ring):
    """Rings 1 .. 4 nside - 1 counted from the north pole: -> (nr, shifted, z, theta, first) -- pixels per quarter (the ring
    holds 4 nr), whether the first centre sits half a step from phi = 0 (the caps, and the belt rings with (ring - nside) even),
    z and theta of the centres (the expressions of ``pix2vec``), RING index of the first pixel."""
    ring = np.asarray(ring, dtype=np.int64)
    fact2 = 4.0 / (12 * nside * nside)
    fact1 = (2 * nside) * fact2
    north = ring < nside
    south = ring > 3 * nside
    nr = np.where(north, ring, np.where(south, 4 * nside - ring, nside))
    nrf = nr.astype(np.float64)
    z = np.where(north, 1.0 - (nrf * nrf) * fact2, np.where(south, (nrf * nrf) * fact2 - 1.0, (2 * nside - ring) * fact1))
    shifted = np.where(north | south, 1, 1 - ((ring - nside) & 1))
    first = np.where(north, 2 * nr * (nr - 1),
                     np.where(south, 12 * nside * nside - 2 * (nr + 1) * nr, 2 * nside * (nside - 1) + (ring - nside) * 4 * nside))
    theta = np.arctan2(np.sqrt(np.maximum(0.0, (1.0 - z) * (1.0 + z))), z)
    return nr, shifted, z, theta, first


def _ring_above(nside, z):
    """The last ring whose centres lie at or north of z (0: above the first ring); healpy's ``ring_above``."""
    z = np.asarray(z, dtype=np.float64)
    az = np.abs(z)
    belt = (nside * (2.0 - 1.5 * np.where(az <= 2.0 / 3.0, z, 0.0))).astype(np.int64)
    iring = (nside * np.sqrt(3.0 * (1.0 - np.minimum(az, 1.0)))).astype(np.int64)
    return np.where(az <= 2.0 / 3.0, belt, np.where(z > 0, iring, 4 * nside - iring - 1))


def _zphi2ring(nside, z, sth, phi):
    """RING index of the pixel that holds the direction (z = cos theta, sth = sin theta >= 0, phi)."""
    z, sth = np.asarray(z, dtype=np.float64), np.asarray(sth, dtype=np.float64)
    tt = np.minimum(_reduce_phi(phi), np.nextafter(_TWOPI, 0.0)) / (0.5 * np.pi)  # [0, 4)
    za = np.abs(z)
    # the belt: the pixel from the two edge lines through the point
    t1 = nside * (0.5 + tt)
    t2 = nside * z * 0.75
    jp = np.floor(t1 - t2).astype(np.int64)
    jm = np.floor(t1 + t2).astype(np.int64)
    ir = nside + 1 + jp - jm  # 1 .. 2 nside + 1
    kshift = 1 - (ir & 1)
    ip = np.mod((jp + jm - nside + kshift + 1) // 2, 4 * nside)
    belt = 2 * nside * (nside - 1) + (ir - 1) * 4 * nside + ip
    # the caps (sin theta instead of sqrt(1 - |z|) close to a pole, where 1 - |z| has lost its digits)
    tp = tt - np.floor(tt)
    tmp = np.where(za < 0.99, nside * np.sqrt(3.0 * (1.0 - np.minimum(za, 1.0))), nside * sth / np.sqrt((1.0 + za) / 3.0))
    jp = (tp * tmp).astype(np.int64)
    jm = ((1.0 - tp) * tmp).astype(np.int64)
    ir = jp + jm + 1  # ring counted from the nearer pole
    ip = np.mod((tt * ir).astype(np.int64), 4 * ir)
    cap = np.where(z > 0, 2 * ir * (ir - 1) + ip, 12 * nside * nside - 2 * ir * (ir + 1) + ip)
    return np.where(za <= 2.0 / 3.0, belt, cap)


def ang2pix(nside, theta, phi, nest=True):
    """The pixel that holds the direction (theta, phi), like ``hp.ang2pix``: int64, NEST ids by default."""
    nside = _check_nside(nside)
    theta = np.asarray(theta, dtype=np.float64)
    if np.any((theta < 0) | (theta > np.pi)):
        raise ValueError("theta outside [0, pi]")
    pix = _zphi2ring(nside, np.cos(theta), np.sin(theta), phi)
    return ring2nest(nside, pix) if nest else pix


def vec2pix(nside, x, y, z, nest=True):
    """The pixel that holds the direction of the vector (x, y, z) (any positive length), like ``hp.vec2pix``."""
    nside = _check_nside(nside)
    x, y, z = (np.asarray(a, dtype=np.float64) for a in (x, y, z))
    s = np.hypot(x, y)
    r = np.hypot(s, z)
    pix = _zphi2ring(nside, z / r, s / r, np.arctan2(y, x))
    return ring2nest(nside, pix) if nest else pix


def pix2ang(nside, pix, nest=True):
    """(theta, phi) of pixel centres, like ``hp.pix2ang``: theta in [0, pi], phi in [0, 2 pi)."""
    nside = _check_nside(nside)
    pix = np.asarray(pix, dtype=np.int64)
    ring_pix = nest2ring(nside, pix) if nest else pix
    # the ring of a RING index: as ring2nest finds it
    npix, ncap = 12 * nside * nside, 2 * nside * (nside - 1)
    north, south = ring_pix < ncap, ring_pix >= npix - ncap
    i_n = (1 + _isqrt(1 + 2 * np.where(north, ring_pix, 0))) >> 1
    i_s = (1 + _isqrt(2 * np.where(south, npix - ring_pix, 1) - 1)) >> 1
    ring = np.where(north, i_n, np.where(south, 4 * nside - i_s, np.where(north | south, 0, ring_pix - ncap) // (4 * nside) + nside))
    nr, shifted, _, theta, first = _ring_info(nside, ring)
    phi = ((ring_pix - first) + 0.5 * shifted) * ((0.5 * np.pi) / nr)
    return theta, phi


def get_interp_weights(nside, theta, phi=None, nest=True):
    """The four pixels around a direction and their bilinear weights, like ``hp.get_interp_weights`` (healpy's ``get_interpol``):
    -> (pix int64 [4, n], weights float64 [4, n]); entries 0, 1 on the ring above the point, 2, 3 on the ring below.  With
    ``phi=None`` the first argument holds pixel ids and their centres are the directions.

    On a ring of n pixels with step dphi: tmp = phi / dphi - shift / 2, i1 = floor(tmp), w1 = (phi - (i1 + shift / 2) dphi) / dphi,
    pixels i1 and i1 + 1 both wrapped modulo n; the two rings are mixed linearly in theta (the mixing weight clamped to [0, 1]: at
    a ring's own latitude the ring above may be named, with weight 1 up to rounding, on the ring meant).  Above the first ring its
    weights are scaled by theta / theta_1 and the rest, (1 - wtheta) / 4 a pixel, goes to all four pixels of ring 1; below the last
    ring likewise.  A column of the result never holds a pixel twice."""
    nside = _check_nside(nside)
    if phi is None:
        theta, phi = pix2ang(nside, theta, nest)
    theta = np.asarray(theta, dtype=np.float64)
    shape = np.broadcast(theta, np.asarray(phi)).shape
    theta, phi = (np.broadcast_to(np.asarray(a, dtype=np.float64), shape).reshape(-1) for a in (theta, phi))
    if np.any((theta < 0) | (theta > np.pi)):
        raise ValueError("theta outside [0, pi]")
    phi = _reduce_phi(phi)
    nl4 = 4 * nside
    ir1 = _ring_above(nside, np.cos(theta))
    ir2 = ir1 + 1
    north, south = ir1 <= 0, ir2 >= nl4
    pix = np.empty((4, theta.shape[0]), dtype=np.int64)
    pos = np.empty((4, theta.shape[0]), dtype=np.int64)
    w = np.empty((4, theta.shape[0]), dtype=np.float64)
    thetas = []
    firsts = []
    for k, ring in enumerate((np.where(north, 1, ir1), np.where(south, nl4 - 1, ir2))):
        nr, shifted, _, th, first = _ring_info(nside, ring)
        n4 = 4 * nr
        dphi = (0.5 * np.pi) / nr
        half = 0.5 * shifted
        fl = np.floor(phi / dphi - half)  # -1 .. n4
        w1 = (phi - (fl + half) * dphi) / dphi
        i1 = np.mod(fl.astype(np.int64), n4)
        pos[2 * k], pos[2 * k + 1] = i1, np.mod(i1 + 1, n4)
        w[2 * k], w[2 * k + 1] = 1.0 - w1, w1
        thetas.append(th)
        firsts.append(first)
    th1, th2 = thetas
    with np.errstate(divide="ignore", invalid="ignore"):
        wt = np.where(north, theta / th2, np.where(south, (theta - th1) / (np.pi - th1), (theta - th1) / (th2 - th1)))
    wt = np.clip(wt, 0.0, 1.0)
    fac_n, fac_s = (1.0 - wt) * 0.25, wt * 0.25
    upper = np.where(north, 0.0, 1.0 - wt)  # what entries 0, 1 keep of their ring weights
    lower = np.where(south, 0.0, wt)
    add01 = np.where(north, fac_n, np.where(south, fac_s, 0.0))
    add23 = add01
    w[0], w[1] = w[0] * upper + add01, w[1] * upper + add01
    w[2], w[3] = w[2] * lower + add23, w[3] * lower + add23
    # the pole branches: all four pixels from the polar ring, the partners two positions on
    pos[0] = np.where(north, (pos[2] + 2) & 3, pos[0])
    pos[1] = np.where(north, (pos[3] + 2) & 3, pos[1])
    pos[2] = np.where(south, (pos[0] + 2) & 3, pos[2])
    pos[3] = np.where(south, (pos[1] + 2) & 3, pos[3])
    pix[0], pix[1] = firsts[0] + pos[0], firsts[0] + pos[1]
    pix[2], pix[3] = firsts[1] + pos[2], firsts[1] + pos[3]
    if nest:
        pix = ring2nest(nside, pix)
    return pix.reshape((4,) + shape), w.reshape((4,) + shape)


def get_interp_val(m, theta, phi, nest=True):
    """The map(s) ``m`` ((npix,) or (k, npix)) interpolated at the directions (theta, phi), like ``hp.get_interp_val``."""
    m = np.asarray(m)
    pix, w = get_interp_weights(npix2nside(m.shape[-1]), theta, phi, nest)
    return (m[..., pix] * w).sum(axis=-1 - (pix.ndim - 1))


def rotation_matrix(alpha, beta, gamma):
    """The ZYZ rotation Rz(alpha) Ry(beta) Rz(gamma), float64 [3, 3]: a map rotated by R has y(v) = x(R^T v)."""
    ca, sa, cb, sb, cg, sg = (f(float(a)) for a in (alpha, beta, gamma) for f in (np.cos, np.sin))
    rz1 = np.array([[ca, -sa, 0.0], [sa, ca, 0.0], [0.0, 0.0, 1.0]])
    ry = np.array([[cb, 0.0, sb], [0.0, 1.0, 0.0], [-sb, 0.0, cb]])
    rz2 = np.array([[cg, -sg, 0.0], [sg, cg, 0.0], [0.0, 0.0, 1.0]])
    return rz1 @ ry @ rz2


def random_rotations(n, generator=None, device=None):
    """``n`` rotations uniform on SO(3): float64 tensor [n, 3, 3] on ``device``.  Normalised quaternions from four normals drawn
    from ``generator`` (a ``torch.Generator`` of that device): reproducible, and drawn on the device without a synchronisation."""
    import torch

    q = torch.randn((int(n), 4), dtype=torch.float64, generator=generator, device=device)
    q = q / torch.linalg.norm(q, dim=1, keepdim=True)
    a, b, c, d = q.unbind(1)
    rows = (a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c),
            2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b),
            2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d)
    return torch.stack(rows, dim=1).reshape(-1, 3, 3)


def rotation_stencil(nside, rot, indices=None):
    """The stencil that rotates a NEST map of the pixel set ``indices`` (None: the full sky) by the matrix ``rot`` [3, 3]:
    -> (rows int64 [4, M], weights float64 [4, M]) with y[r] = sum_j weights[j, r] x[rows[j, r]] -- the interpolation weights at
    R^T v(indices[r]); a source pixel outside the set has row -1 (it contributes zero, nothing is renormalised)."""
    nside = _check_nside(nside)
    ind = _index_set(nside, indices)
    rot = np.asarray(rot, dtype=np.float64)
    if rot.shape != (3, 3):
        raise ValueError("rot must be a [3, 3] matrix")
    u = pix2vec(nside, ind) @ rot  # rows R^T v
    s = np.hypot(u[:, 0], u[:, 1])
    pix, w = get_interp_weights(nside, np.arctan2(s, u[:, 2]), np.arctan2(u[:, 1], u[:, 0]))
    if ind is not None:
        lut = np.full(nside2npix(nside), -1, dtype=np.int64)
        lut[ind] = np.arange(ind.shape[0], dtype=np.int64)
        pix = lut[pix]
    return pix, w


# ----------------------------------------------------------------------------------------------
# Spherical harmonic transforms, numpy, healpy's names (map2alm, alm2map, alm2cl, anafast, almxfl): the reference of the kernels
# of csrc/healpix_sht.hip and what deepsphere/sht.py runs on CPU tensors.  Equal pixel weights (healpy with use_weights=False).
# The Legendre functions come from the plain three-term recurrence in np.longdouble, whose exponent range (the 80-bit x87 format:
# smallest normal 3e-4932) holds sin^m theta without the rescaling the kernel needs, so the two share no trick; sums over pixels,
# rings and l run in float64.  NOTE: nest=True is this module's default everywhere; healpy's is nest=False.
# ----------------------------------------------------------------------------------------------

def alm_size(lmax):
    """Number of coefficients of healpy's packed layout with mmax = lmax: (lmax + 1)(lmax + 2) / 2, like ``hp.Alm.getsize``."""
    lmax = int(lmax)
    if lmax < 0:
        raise ValueError(f"lmax = {lmax} is negative")
    return (lmax + 1) * (lmax + 2) // 2


def alm_index(lmax, l, m):
    """Index of a_lm (0 <= m <= l <= lmax) in healpy's packed layout, m-major: m (2 lmax + 1 - m) / 2 + l, like ``hp.Alm.getidx``."""
    l, m = np.asarray(l, dtype=np.int64), np.asarray(m, dtype=np.int64)
    return m * (2 * int(lmax) + 1 - m) // 2 + l


def _alm_lmax(nalm):
    lmax = (int(np.sqrt(8 * int(nalm) + 1)) - 3) // 2
    if alm_size(lmax) != int(nalm):
        raise ValueError(f"{nalm} coefficients are not (lmax + 1)(lmax + 2) / 2 for any lmax")
    return lmax


def _sht_lmax(nside, lmax):
    lmax = 3 * nside - 1 if lmax is None else int(lmax)
    if lmax < 0 or lmax > 4 * nside - 1:
        raise ValueError(f"lmax = {lmax} outside [0, 4 nside - 1 = {4 * nside - 1}]")
    return lmax


def legendre_lambda(nside, m, lmax, dtype=np.float64):
    """The normalised associated Legendre functions lambda_lm(cos theta) (Y_lm = lambda_lm e^{i m phi}) at the 4 nside - 1 rings of
    ``nside`` for l = m .. lmax: -> [lmax + 1 - m, 4 nside - 1] in ``dtype``, computed in np.longdouble by
    lambda_mm = (-1)^m sqrt((2 m + 1) / (4 pi) prod_{k <= m} (2 k - 1) / (2 k)) sin^m theta, lambda_{m+1,m} = x sqrt(2 m + 3) lambda_mm,
    lambda_lm = a_lm (x lambda_{l-1,m} - lambda_{l-2,m} / a_{l-1,m}), a_lm = sqrt((4 l^2 - 1) / (l^2 - m^2)).  The northern rings and
    the equator are computed, the southern ones follow from lambda_lm(pi - theta) = (-1)^(l + m) lambda_lm(theta)."""
    nside, m, lmax = _check_nside(nside), int(m), int(lmax)
    if not 0 <= m <= lmax:
        raise ValueError(f"m = {m} outside [0, lmax = {lmax}]")
    ld = np.longdouble
    _, _, z, _, _ = _ring_info(nside, np.arange(1, 2 * nside + 1))
    x = z.astype(ld)
    st = np.sqrt(np.maximum(ld(0), (ld(1) - x) * (ld(1) + x)))
    k = np.arange(1, m + 1, dtype=ld)
    pref = np.sqrt(ld(2 * m + 1) / (ld(4) * ld(np.pi)) * np.prod((2 * k - 1) / (2 * k)))
    out = np.empty((lmax + 1 - m, 4 * nside - 1), dtype=dtype)
    sign = np.where((np.arange(m, lmax + 1) - m) & 1, -1.0, 1.0)
    lam2 = np.zeros_like(x)
    with np.errstate(under="ignore"):
        lam1 = (ld(-1) if m & 1 else ld(1)) * pref * st ** m
        a1 = ld(0)
        for l in range(m, lmax + 1):
            if l > m:
                a = np.sqrt(ld(4 * l * l - 1) / ld(l * l - m * m))
                lam1, lam2 = a * (x * lam1 - (lam2 / a1 if l > m + 1 else ld(0))), lam1
                a1 = a
            row = lam1.astype(dtype)
            out[l - m, :2 * nside] = row
            out[l - m, 2 * nside:] = sign[l - m] * row[2 * nside - 2::-1]
    return out


def _ring_phase0(nside):
    """Per ring 1 .. 4 nside - 1: (nr, first RING index, e^{-i phi_0 m} as a function of m) ingredients: phi of the first pixel is
    (1 - kshift) / (8 nr) of a turn, kshift = 1 - shifted."""
    nr, shifted, _, _, first = _ring_info(nside, np.arange(1, 4 * nside))
    return nr, 1 - shifted, first


def _ring_transform(ringmaps, nside, lmax):
    """F_m(ring) = sum_j x[ring, j] e^{-i m phi_j} of RING-ordered float64 maps [npix, F], m <= lmax: -> complex128 [lmax + 1, 4 nside - 1, F].
    One FFT per ring; m at or above the ring's length folds onto m mod 4 nr; the phase of the ring's first pixel, m (1 - kshift) of
    8 nr-ths of a turn, is reduced in integers."""
    nr, kshift, first = _ring_phase0(nside)
    m = np.arange(lmax + 1, dtype=np.int64)
    F = ringmaps.shape[1]
    out = np.empty((lmax + 1, 4 * nside - 1, F), dtype=np.complex128)
    for r in range(4 * nside - 1):
        n4 = 4 * int(nr[r])
        f = np.fft.fft(ringmaps[first[r]:first[r] + n4], axis=0)
        k0 = (m * (1 - int(kshift[r]))) % (2 * n4)
        out[:, r] = f[m % n4] * np.exp(-2j * np.pi * (k0 / (2.0 * n4)))[:, None]
    return out


def _ring_synthesis(fm, nside):
    """The transpose: RING-ordered float64 maps [npix, F] = Re sum_m c_m F_m(ring) e^{+i m phi_j}, c_0 = 1, c_m = 2."""
    nr, kshift, first = _ring_phase0(nside)
    lmax, F = fm.shape[0] - 1, fm.shape[2]
    m = np.arange(lmax + 1, dtype=np.int64)
    mult = np.where(m == 0, 1.0, 2.0)[:, None]
    out = np.empty((12 * nside * nside, F), dtype=np.float64)
    for r in range(4 * nside - 1):
        n4 = 4 * int(nr[r])
        k0 = (m * (1 - int(kshift[r]))) % (2 * n4)
        g = np.zeros((n4, F), dtype=np.complex128)
        np.add.at(g, m % n4, fm[:, r] * mult * np.exp(2j * np.pi * (k0 / (2.0 * n4)))[:, None])
        out[first[r]:first[r] + n4] = np.fft.ifft(g, axis=0).real * n4
    return out


def _as_maps(maps, nest):
    maps = np.asarray(maps, dtype=np.float64)
    one = maps.ndim == 1
    m2 = maps.reshape(maps.shape[0], -1) if not one else maps[:, None]
    if maps.ndim > 2:
        raise ValueError("maps must be (npix,) or (npix, F)")
    nside = _check_nside(npix2nside(m2.shape[0]))
    if nest:
        m2 = m2[ring2nest(nside, np.arange(m2.shape[0], dtype=np.int64))]
    return m2, nside, one


def _analysis(ringmaps, nside, lmax):
    """Plain quadrature with w = 4 pi / npix of RING-ordered [npix, F] maps -> complex128 [nalm, F]."""
    fm = _ring_transform(ringmaps, nside, lmax)
    w = 4.0 * np.pi / (12 * nside * nside)
    alm = np.empty((alm_size(lmax), ringmaps.shape[1]), dtype=np.complex128)
    for m in range(lmax + 1):
        i0 = int(alm_index(lmax, m, m))
        alm[i0:i0 + lmax + 1 - m] = w * (legendre_lambda(nside, m, lmax) @ fm[m])
    return alm


def _synthesis(alm, nside, lmax):
    """RING-ordered float64 [npix, F] maps of complex128 [nalm, F] coefficients."""
    fm = np.empty((lmax + 1, 4 * nside - 1, alm.shape[1]), dtype=np.complex128)
    for m in range(lmax + 1):
        i0 = int(alm_index(lmax, m, m))
        fm[m] = legendre_lambda(nside, m, lmax).T @ alm[i0:i0 + lmax + 1 - m]
    return _ring_synthesis(fm, nside)


def map2alm(maps, lmax=None, iter=3, nest=True):  # noqa: A002  (healpy's argument name)
    """The spherical harmonic coefficients of the map(s) ``maps`` ((npix,) or (npix, F)), like ``hp.map2alm(use_weights=False)``:
    -> complex128 (nalm,) or (nalm, F) in healpy's packed layout (``alm_index``), mmax = lmax, lmax = 3 nside - 1 by default.
    ``iter = 0``: the quadrature a_lm = w sum_p Y*_lm(p) x_p with equal weights w = 4 pi / npix; ``iter > 0`` adds healpy's Jacobi
    steps alm += map2alm(map - alm2map(alm), iter=0).  ``nest=True`` (NEST-ordered input) is the default here and is NOT healpy's."""
    m2, nside, one = _as_maps(maps, nest)
    lmax = _sht_lmax(nside, lmax)
    alm = _analysis(m2, nside, lmax)
    for _ in range(int(iter)):
        alm += _analysis(m2 - _synthesis(alm, nside, lmax), nside, lmax)
    return alm[:, 0] if one else alm


def alm2map(alm, nside, nest=True):
    """The map(s) of the coefficients ``alm`` ((nalm,) or (nalm, F), packed, mmax = lmax), like ``hp.alm2map``: float64 (npix,) or
    (npix, F); the m = 0 terms count once, the m > 0 terms as 2 Re.  ``nest=True`` (NEST-ordered output) is the default here and
    is NOT healpy's."""
    nside = _check_nside(nside)
    alm = np.asarray(alm, dtype=np.complex128)
    one = alm.ndim == 1
    if alm.ndim > 2:
        raise ValueError("alm must be (nalm,) or (nalm, F)")
    a2 = alm[:, None] if one else alm
    lmax = _alm_lmax(a2.shape[0])
    _sht_lmax(nside, lmax)
    out = _synthesis(a2, nside, lmax)
    if nest:
        out = out[nest2ring(nside, np.arange(out.shape[0], dtype=np.int64))]
    return out[:, 0] if one else out


def alm2cl(alm):
    """The auto power spectrum C_l = (|a_l0|^2 + 2 sum_{m > 0} |a_lm|^2) / (2 l + 1) of packed ``alm`` ((nalm,) or (nalm, F)), like
    ``hp.alm2cl``: float64 (lmax + 1,) or (lmax + 1, F)."""
    alm = np.asarray(alm, dtype=np.complex128)
    lmax = _alm_lmax(alm.shape[0])
    p = alm.real ** 2 + alm.imag ** 2
    cl = np.zeros((lmax + 1,) + alm.shape[1:], dtype=np.float64)
    for m in range(lmax + 1):
        i0 = int(alm_index(lmax, m, m))
        cl[m:] += (1.0 if m == 0 else 2.0) * p[i0:i0 + lmax + 1 - m]
    return cl / (2.0 * np.arange(lmax + 1).reshape((-1,) + (1,) * (alm.ndim - 1)) + 1.0)


def anafast(maps, lmax=None, iter=3, nest=True):  # noqa: A002
    """The auto power spectrum of the map(s), ``alm2cl(map2alm(maps, lmax, iter, nest))``, like ``hp.anafast(use_weights=False)`` for
    one map.  ``nest=True`` is the default here and is NOT healpy's."""
    return alm2cl(map2alm(maps, lmax=lmax, iter=iter, nest=nest))


def almxfl(alm, fl):
    """``alm`` ((nalm,) or (nalm, F)) with every a_lm multiplied by ``fl[l]`` (l beyond len(fl): by zero), like ``hp.almxfl``."""
    alm = np.asarray(alm, dtype=np.complex128)
    lmax = _alm_lmax(alm.shape[0])
    fl = np.asarray(fl)
    full = np.zeros(lmax + 1, dtype=fl.dtype)
    n = min(lmax + 1, fl.shape[0])
    full[:n] = fl[:n]
    ls = np.concatenate([np.arange(m, lmax + 1) for m in range(lmax + 1)])
    return alm * full[ls].reshape((-1,) + (1,) * (alm.ndim - 1))
