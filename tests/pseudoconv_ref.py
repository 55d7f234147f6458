"""Float64 numpy yardstick of the pseudo-convolutions' row GEMM (not collected by pytest):
    Y[r, c] = act(sum_j X[r, j] W[j, c] + b[c mod P]),   X (R, Kd), W (Kd, C), b (P) or None
and of its gradients, with the derivative of the activation taken from the stored output as the kernels do."""

import numpy as np


def _act(z, act):
    if act in (None, "none", "linear"):
        return z
    if act == "relu":
        return np.maximum(z, 0.0)
    if act == "elu":
        return np.where(z > 0, z, np.expm1(np.minimum(z, 0.0)))
    if act == "sigmoid":
        return 1.0 / (1.0 + np.exp(-z))
    if act == "tanh":
        return np.tanh(z)
    raise ValueError(act)


def _act_grad_from_output(y, act):
    if act in (None, "none", "linear"):
        return np.ones_like(y)
    if act == "relu":
        return (y > 0).astype(np.float64)
    if act == "elu":
        return np.where(y > 0, 1.0, y + 1.0)
    if act == "sigmoid":
        return y * (1.0 - y)
    if act == "tanh":
        return 1.0 - y * y
    raise ValueError(act)


def patch_forward(X, W, b, P, act):
    X, W = np.asarray(X, dtype=np.float64), np.asarray(W, dtype=np.float64)
    C = W.shape[1]
    assert C % P == 0
    z = X @ W
    if b is not None:
        z = z + np.tile(np.asarray(b, dtype=np.float64), C // P)
    return _act(z, act)


def patch_backward(X, W, Y, dY, P, act):
    """-> dX, dW, db from the stored output Y."""
    X, W, Y, dY = (np.asarray(v, dtype=np.float64) for v in (X, W, Y, dY))
    dZ = dY * _act_grad_from_output(Y, act)
    R, C = dZ.shape
    return dZ @ W.T, X.T @ dZ, dZ.reshape(R, C // P, P).sum(axis=(0, 1))


def conv_image(weight):
    """HealpyPseudoConv: filter.weight (Fout, Fin, g) -> W (g Fin, Fout), W[i Fin + f, o] = weight[o, f, i]."""
    weight = np.asarray(weight)
    return np.transpose(weight, (2, 1, 0)).reshape(-1, weight.shape[0])


def conv_transpose_image(weight):
    """HealpyPseudoConv_Transpose: filter.weight (Fin, Fout, g) -> W (Fin, g Fout), W[f, i Fout + o] = weight[f, o, i]."""
    weight = np.asarray(weight)
    return np.transpose(weight, (0, 2, 1)).reshape(weight.shape[0], -1)


def conv_image_inverse(W, Fin, g):
    """dW (g Fin, Fout) -> the layout of filter.weight (Fout, Fin, g)."""
    W = np.asarray(W)
    return np.transpose(W.reshape(g, Fin, W.shape[1]), (2, 1, 0))


def conv_transpose_image_inverse(W, Fout, g):
    """dW (Fin, g Fout) -> the layout of filter.weight (Fin, Fout, g)."""
    W = np.asarray(W)
    return np.transpose(W.reshape(W.shape[0], g, Fout), (0, 2, 1))


def make_data(R, Kd, C, P, seed=0):
    """X ~ N(0, 1), W ~ N(0, 1) / sqrt(Kd), b = 0.3 N(0, 1), dY ~ N(0, 1), all float32."""
    rng = np.random.default_rng([seed, R, Kd, C, P])
    X = rng.standard_normal((R, Kd)).astype(np.float32)
    W = (rng.standard_normal((Kd, C)) / np.sqrt(Kd)).astype(np.float32)
    b = (0.3 * rng.standard_normal(P)).astype(np.float32)
    dY = rng.standard_normal((R, C)).astype(np.float32)
    return X, W, b, dY
