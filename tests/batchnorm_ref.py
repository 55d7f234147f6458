"""The float64 yardstick of the batch-norm kernels (csrc/batch_norm.hip), plain numpy (not collected by pytest).

Channels-last maps ``(rows, F)``; any leading axes are flattened into the rows.  ``act`` is one of ``ACTS``:
    z = act(x^ * gamma + shift),   x^ = (y - mean) / sqrt(var + eps),   mean and (biased) var per channel over the rows.
"""

import numpy as np

ACTS = ("none", "relu", "elu", "sigmoid", "tanh")  # in the order of the DSPH_ACT_* codes 0 .. 4


def _rows(a):
    a = np.asarray(a, dtype=np.float64)
    return a.reshape(-1, a.shape[-1])


def _vec(v, F, neutral):
    return np.full(F, neutral, dtype=np.float64) if v is None else np.asarray(v, dtype=np.float64).reshape(F)


def _act(v, act):
    if act == "none":
        return v
    if act == "relu":
        return np.maximum(v, 0.0)
    if act == "elu":
        return np.where(v > 0.0, v, np.expm1(np.minimum(v, 0.0)))
    if act == "sigmoid":
        return 1.0 / (1.0 + np.exp(-v))
    if act == "tanh":
        return np.tanh(v)
    raise ValueError(act)


def _act_grad_from_output(z, act):
    """d act / d (pre-activation), written in terms of the activation's output z."""
    if act == "none":
        return np.ones_like(z)
    if act == "relu":
        return (z > 0.0).astype(np.float64)
    if act == "elu":
        return np.where(z > 0.0, 1.0, z + 1.0)
    if act == "sigmoid":
        return z * (1.0 - z)
    if act == "tanh":
        return 1.0 - z * z
    raise ValueError(act)


def bn_forward(y, eps, gamma=None, shift=None, act="none"):
    """-> (mean [F], var [F] (biased), z of y's shape), all float64."""
    shape = np.shape(y)
    y2 = _rows(y)
    F = y2.shape[1]
    mean = y2.mean(axis=0)
    var = ((y2 - mean) ** 2).mean(axis=0)
    xhat = (y2 - mean) / np.sqrt(var + eps)
    z = _act(xhat * _vec(gamma, F, 1.0) + _vec(shift, F, 0.0), act)
    return mean, var, z.reshape(shape)


def bn_backward(y, dz, eps, gamma=None, shift=None, act="none", z_for_mask=None):
    """-> (dy of y's shape, dgamma [F], dshift [F]) of ``bn_forward`` under the upstream gradient ``dz``, float64.

    ``z_for_mask``: for relu the derivative mask is taken from THIS output (the z under test) instead of the yardstick's own: an
    element within rounding of the kink must not flip a mask -- one flip moves dshift by a whole |dz| -- and z itself is held to
    the forward tolerance separately.  The smooth activations always use the yardstick's own z."""
    shape = np.shape(y)
    y2, dz2 = _rows(y), _rows(dz)
    R, F = y2.shape
    g_ = _vec(gamma, F, 1.0)
    mean = y2.mean(axis=0)
    var = ((y2 - mean) ** 2).mean(axis=0)
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = (y2 - mean) * rstd
    z = _act(xhat * g_ + _vec(shift, F, 0.0), act)
    if act == "relu" and z_for_mask is not None:
        z = _rows(z_for_mask)
    g = dz2 * _act_grad_from_output(z, act)
    s1 = g.sum(axis=0)
    s2 = (g * xhat).sum(axis=0)
    dy = g_ * rstd * (g - s1 / R - xhat * s2 / R)
    return dy.reshape(shape), s2, s1


def moving_update(running_mean, running_var, mean, var, rows, momentum):
    """The moving statistics after one training call, as ``torch.nn.BatchNorm1d`` keeps them: running = (1 - m) running + m batch,
    the variance with the UNBIASED batch variance var * rows / (rows - 1).  -> (running_mean, running_var), float64."""
    rm = (1.0 - momentum) * np.asarray(running_mean, dtype=np.float64) + momentum * np.asarray(mean, dtype=np.float64)
    unbiased = np.asarray(var, dtype=np.float64) * rows / (rows - 1.0)
    rv = (1.0 - momentum) * np.asarray(running_var, dtype=np.float64) + momentum * unbiased
    return rm, rv
