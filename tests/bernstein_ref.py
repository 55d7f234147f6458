"""Float64 numpy restatement of the Bernstein graph convolution for the tests (not collected by pytest).

The oracle is the reference's op sequence (``Bernstein.call``, gnn_layers.py:537-561), restated here: for every i in 0 .. K the
input is multiplied i times by L~, then K - i times by (2 I - L~), then by theta_i = binom(K, i) / 2^K -- EXCEPT that for
i = K the second loop runs zero times and the reference scales what that loop left behind for i = K - 1 (the already scaled
plane K - 1) once more: plane K = theta_K * plane K-1.  ``planes`` does exactly that.

TensorFlow is not available where these tests were written, so no golden file could be produced by running the reference
itself; the tests compare against this restatement, with ``Lt`` the layer's own fp32 L~ widened to float64 (``csr``), so only
the arithmetic is compared.
"""

from math import comb

import numpy as np
from scipy import sparse


def csr(cols, vals):
    """The padded ELL arrays of a layer ([M, W]: int32 columns, fp32 values) as a float64 CSR matrix."""
    cols, vals = np.asarray(cols), np.asarray(vals, dtype=np.float64)
    M, W = cols.shape
    A = sparse.csr_matrix((vals.reshape(-1), cols.reshape(-1).astype(np.int64), np.arange(0, M * W + 1, W)), shape=(M, M))
    A.sum_duplicates()
    return A


def _apply(Lt, v):
    """Lt over the pixel axis of v (N, M, F)."""
    N, M, F = v.shape
    flat = v.transpose(1, 0, 2).reshape(M, N * F)
    return np.asarray(Lt @ flat).reshape(M, N, F).transpose(1, 0, 2)


def planes(Lt, x, K):
    """The K + 1 planes the reference stacks, (N, M, Fin, K + 1) in float64."""
    Lt = sparse.csr_matrix(Lt, dtype=np.float64) if sparse.issparse(Lt) else np.asarray(Lt, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    out = []
    left = None  # what the loop over K - i last produced: kept across i, like the reference's x3
    for i in range(K + 1):
        theta = comb(K, i) / 2.0**K
        cur = x
        for _ in range(i):
            cur = _apply(Lt, cur)
        for _ in range(K - i):
            left = 2.0 * cur - _apply(Lt, cur)
            cur = left
        left = theta * left
        out.append(left)
    return np.stack(out, axis=-1)


def forward(Lt, x, kernel, K):
    """y[n, m, o] = sum_{f, i} planes[n, m, f, i] kernel[f*(K+1) + i, o]: no bias, no batch norm, no activation."""
    P = planes(Lt, x, K)
    N, M, Fin, Kp = P.shape
    return (P.reshape(N * M, Fin * Kp) @ np.asarray(kernel, dtype=np.float64)).reshape(N, M, -1)


def grad_x(Lt, kernel, K, dy):
    """d<y, dy>/dx: every plane is a polynomial in L~ acting on the pixel axis, so its adjoint is the same polynomial in L~^T and
    commutes with the contraction over channels."""
    Lt = sparse.csr_matrix(Lt, dtype=np.float64) if sparse.issparse(Lt) else np.asarray(Lt, dtype=np.float64)
    P = planes(Lt.T, dy, K)  # (N, M, Fout, K + 1)
    Fout = P.shape[2]
    W = np.asarray(kernel, dtype=np.float64).reshape(-1, K + 1, Fout)  # (Fin, K + 1, Fout)
    return np.einsum("nmoi,fio->nmf", P, W)


def grad_w(Lt, x, K, dy):
    """d<y, dy>/dkernel, [(K+1) * Fin, Fout]."""
    P = planes(Lt, x, K)
    N, M, Fin, Kp = P.shape
    return P.reshape(N * M, Fin * Kp).T @ np.asarray(dy, dtype=np.float64).reshape(N * M, -1)
