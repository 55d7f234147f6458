"""Float64 numpy restatement of HealpySmoothing for the tests (not collected by pytest): the passes on a given table, one pass
as ``_native.ell_smooth`` documents it (empty slots included), the all-pairs construction of the kernel, and the dense matrix of a
table for the gradient."""

import numpy as np

from deepsphere import healpix


def n_passes(reps):
    return 1 if reps is None else int(np.max(reps))


def apply(cols, vals, x, reps=None, mask=None):
    """The layer's passes on the fp32 table (cols, vals) [M, W] with float64 sums: channel c is multiplied by the matrix
    reps[c] times (once when reps is None), then the result by the mask ((M,), (M, 1) or (M, C))."""
    cols, vals = np.asarray(cols), np.asarray(vals, dtype=np.float64)
    y = np.array(x, dtype=np.float64)
    N, M, C = y.shape
    for c in range(C):
        for _ in range(1 if reps is None else int(reps[c])):
            y[:, :, c] = (y[:, :, c][:, cols] * vals[None]).sum(axis=-1)
    if mask is not None:
        m = np.asarray(mask, dtype=np.float64)
        y = y * (m[None, :, None] if m.ndim == 1 else m[None])
    return y


def apply_pass(cols, vals, x, reps=None, pass_index=0, mask=None):
    """ONE pass as ``_native.ell_smooth`` documents it, with float64 sums: out[n, m, c] = sum_j vals[m, j] x[n, cols[m, j], c] for
    the channels with reps[c] > pass_index (all of them when reps is None), x[n, m, c] for the others, times the mask ((M, 1) or
    (M, C)) when one is given.  A table entry outside [0, M) is an empty slot: weight 0, whatever ``vals`` holds there (``apply``
    indexes with the raw columns, where a -1 wraps to the last pixel)."""
    cols, vals = np.asarray(cols).astype(np.int64), np.asarray(vals, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    N, M, C = x.shape
    ok = (cols >= 0) & (cols < M)
    w = np.where(ok, vals, 0.0)
    safe = np.where(ok, cols, 0)
    y = x.copy()
    for c in range(C):
        if reps is None or int(reps[c]) > pass_index:
            y[:, :, c] = (x[:, :, c][:, safe] * w[None]).sum(axis=-1)
    if mask is not None:
        m = np.asarray(mask, dtype=np.float64)
        assert m.shape in ((M, 1), (M, C))
        y = y * m[None]
    return y


def dense(cols, vals):
    """The table as a dense float64 matrix K, K[m, cols[m, j]] += vals[m, j]."""
    cols, vals = np.asarray(cols), np.asarray(vals, dtype=np.float64)
    M = cols.shape[0]
    K = np.zeros((M, M))
    np.add.at(K, (np.repeat(np.arange(M), cols.shape[1]), cols.reshape(-1)), vals.reshape(-1))
    return K


def apply_transposed(K, g, reps=None, mask=None):
    """The input gradient: channel c of (g times mask) multiplied reps[c] times by K^T."""
    g = np.array(g, dtype=np.float64)
    if mask is not None:
        m = np.asarray(mask, dtype=np.float64)
        g = g * (m[None, :, None] if m.ndim == 1 else m[None])
    for c in range(g.shape[2]):
        for _ in range(1 if reps is None else int(reps[c])):
            g[:, :, c] = g[:, :, c] @ K  # (K^T v)^T = v^T K
    return g


def brute_table(nside, indices, sigma_rad, n_sigma):
    """All pairs: -> (theta [M, M] great-circle distances, W = the largest number of pixels within n_sigma * sigma_rad of a
    pixel (<=, the pixel itself included), d_k [M] = the W-th smallest distance of every row, kern [M, M] = the float64 kernel
    exp(-theta^2 / (2 sigma^2)))."""
    v = healpix.pix2vec(nside, np.asarray(indices, dtype=np.int64))
    d2 = np.zeros((v.shape[0], v.shape[0]))
    for k in range(3):
        d2 += (v[:, None, k] - v[None, :, k]) ** 2
    theta = 2.0 * np.arcsin(np.minimum(0.5 * np.sqrt(d2), 1.0))  # chord -> angle: exact for small angles, unlike arccos
    W = int((theta <= n_sigma * sigma_rad).sum(axis=1).max())
    d_k = np.sort(theta, axis=1)[:, W - 1]
    return theta, W, d_k, np.exp(-0.5 * (theta / sigma_rad) ** 2)
