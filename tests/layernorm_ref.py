"""Float64 restatement of the layer norm with the residual add in front (``dsph_ln_forward`` / ``dsph_ln_backward``): the yardstick
of tests/test_gpu_layernorm.py (not collected by pytest; held to torch's float64 autograd at 1e-12 and to ``oracle.keras_layer_norm``
by tests/test_layernorm_host.py)."""

import numpy as np


def ln_forward(x, eps, gamma=None, beta=None, res=None):
    """-> (z, a): a = x + res (x itself without res), z = (a - mean) / sqrt(var + eps) * gamma + beta over the trailing axis, the
    variance biased.  Inputs of any float type; everything is evaluated in float64."""
    a = np.asarray(x, dtype=np.float64)
    if res is not None:
        a = a + np.asarray(res, dtype=np.float64)
    mean = a.mean(axis=-1, keepdims=True)
    var = ((a - mean) ** 2).mean(axis=-1, keepdims=True)
    z = (a - mean) / np.sqrt(var + float(eps))
    if gamma is not None:
        z = z * np.asarray(gamma, dtype=np.float64)
    if beta is not None:
        z = z + np.asarray(beta, dtype=np.float64)
    return z, a


def ln_backward(a, dz, eps, gamma=None, dsum=None):
    """-> (da, dgamma, dbeta) from the normalised input a, the gradient dz of z and the gradient dsum that reached the sum output:
    g = dz gamma, da = rstd (g - mean_d(g) - x^ mean_d(g x^)) + dsum, dgamma = sum_r dz x^, dbeta = sum_r dz."""
    a = np.asarray(a, dtype=np.float64)
    dz = np.asarray(dz, dtype=np.float64)
    d = a.shape[-1]
    mean = a.mean(axis=-1, keepdims=True)
    var = ((a - mean) ** 2).mean(axis=-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + float(eps))
    xh = (a - mean) * rstd
    g = dz if gamma is None else dz * np.asarray(gamma, dtype=np.float64)
    da = rstd * (g - g.mean(axis=-1, keepdims=True) - xh * (g * xh).mean(axis=-1, keepdims=True))
    if dsum is not None:
        da = da + np.asarray(dsum, dtype=np.float64)
    return da, (dz * xh).reshape(-1, d).sum(axis=0), dz.reshape(-1, d).sum(axis=0)


def make_data(rows, d, seed=None):
    """The data of the GPU tests, float32: rows of N(0, 1) shifted by 0, +10 and -3 in turn, row 4 constant; res, dz, dsum N(0, 1);
    gamma = 1 + 0.2 N, beta = 0.3 N.  x + res carries the shifts (res has none), so the normalised rows do in either form."""
    rng = np.random.default_rng(1000 * d + rows if seed is None else seed)
    x = rng.standard_normal((rows, d)) + np.array([0.0, 10.0, -3.0])[np.arange(rows) % 3][:, None]
    res = rng.standard_normal((rows, d))
    if rows > 4:
        x[4] = 1.5
        res[4] = -0.25
    dz = rng.standard_normal((rows, d))
    dsum = rng.standard_normal((rows, d))
    gamma = 1.0 + 0.2 * rng.standard_normal(d)
    beta = 0.3 * rng.standard_normal(d)
    return tuple(v.astype(np.float32) for v in (x, res, dz, dsum, gamma, beta))
