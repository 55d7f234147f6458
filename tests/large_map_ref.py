"""Checker of the large-map tests (tests/test_gpu_large_maps.py; not collected by pytest): float64 references in plain torch,
walked over a map in chunks of rows ON THE TENSOR'S OWN DEVICE, because no host reference of a 2e9-element map comes back in
seconds.  Everything here takes CPU tensors as well; tests/test_large_maps_host.py proves on small CPU tensors that the checker
reports planted faults and that these references equal the suite's numpy yardsticks to 1e-12.

Error measure: max|got - ref| / max|ref| over the WHOLE map, ``helpers.rel_err``'s.  ``sweep`` returns the two maxima.
"""

import math

import numpy as np
import torch

CHUNK_ELEMS = 1 << 26     # elements of a map per chunk of a sweep
BAND = 4096               # floats of a sentinel band (16 KiB: a view behind it keeps its 16-byte alignment)
SENTINEL = -6.02214076e23  # what the bands hold: no result of any test comes near it
ACTS = ("none", "relu", "elu", "sigmoid", "tanh")  # in the order of the DSPH_ACT_* codes 0 .. 4


def chunk_rows(width, elems=CHUNK_ELEMS):
    """Rows of ``width`` elements that make one chunk."""
    return max(1, elems // max(int(width), 1))


def spans(rows, step):
    for r0 in range(0, int(rows), int(step)):
        yield r0, min(r0 + int(step), int(rows))


# ---- the sweep -----------------------------------------------------------------------------------------------------------------

class Accum:
    """max|got - ref|, max|ref| and the place of the largest error over the chunks handed to ``add``; a NaN in ``got`` (the value
    every output is pre-filled with) or any other non-finite number fails at once, naming the first row that holds one."""

    def __init__(self, what="map"):
        self.what, self.err, self.scale, self.worst_row, self.elems = what, 0.0, 0.0, -1, 0

    def add(self, got, ref, row0=0):
        got2 = got.reshape(got.shape[0], -1) if got.dim() > 1 else got.reshape(-1, 1)
        ref2 = ref.reshape(got2.shape).to(torch.float64)
        bad = ~torch.isfinite(got2)
        if bool(bad.any()):
            r = int(torch.nonzero(bad.any(dim=1))[0, 0])
            kind = "still holds its NaN pre-fill (never written)" if bool(torch.isnan(got2[r]).any()) else "is not finite"
            raise AssertionError(f"{self.what}: row {row0 + r} {kind}; {int(bad.sum())} such elements in rows [{row0}, {row0 + got2.shape[0]})")
        d = (got2.to(torch.float64) - ref2).abs()
        e = float(d.max()) if d.numel() else 0.0
        if e > self.err:
            self.err, self.worst_row = e, row0 + int(torch.argmax(d.max(dim=1).values))
        if ref2.numel():
            self.scale = max(self.scale, float(ref2.abs().max()))
        self.elems += got2.numel()

    @property
    def rel(self):
        return self.err / max(self.scale, 1e-300)


def sweep(got, ref_fn, step, what="map"):
    """``got`` (rows, ...) against ``ref_fn(r0, r1)`` (the float64 reference of got[r0:r1]) over ALL rows, ``step`` rows at a time:
    -> (max|got - ref|, max|ref|).  Fails if an element of ``got`` still holds the NaN it was pre-filled with."""
    acc = Accum(what)
    for r0, r1 in spans(got.shape[0], step):
        acc.add(got[r0:r1], ref_fn(r0, r1), r0)
    assert acc.elems == got.numel()
    return acc.err, acc.scale


def equal_sweep(got, ref_fn, step, what="map"):
    """Bit-for-bit: the number of elements of ``got`` whose bits differ from ``ref_fn(r0, r1)`` (a float32 tensor), over all rows."""
    diff = 0
    for r0, r1 in spans(got.shape[0], step):
        g, r = got[r0:r1].contiguous(), ref_fn(r0, r1).to(torch.float32).contiguous()
        assert bool(torch.isfinite(g).all()), f"{what}: NaN pre-fill (or another non-finite number) left in rows [{r0}, {r1})"
        diff += int((g.view(torch.int32) != r.view(torch.int32)).sum())
    return diff


def chunked_sum(fn, rows, step):
    """sum over all rows of ``fn(r0, r1)`` (a float64 (r1 - r0, ...) tensor), per trailing index: the reductions' reference."""
    total = None
    for r0, r1 in spans(rows, step):
        s = fn(r0, r1).to(torch.float64).sum(dim=0)
        total = s if total is None else total + s
    return total


# ---- windows: rows on the host against the numpy yardsticks -------------------------------------------------------------------------

def window_rows(rows, width, seams=(), n_random=32, seed=0, reach=2):
    """The rows a window check visits, sorted and unique: the first and the last ``2 reach`` rows (the ragged tail), ``reach`` rows
    either side of the elements at offsets 2^29, 2^30 and 2^31 of a (rows, width) map (byte offsets 2^31, 2^32, 2^33) where the map
    reaches them, ``reach`` rows either side of every row of ``seams`` (the first row of a work item: the row before it ends the
    item in front), and ``n_random`` seeded random rows."""
    rows, width = int(rows), int(width)
    out = list(range(min(2 * reach, rows))) + list(range(max(rows - 2 * reach, 0), rows))
    centres = [(1 << p) // width for p in (29, 30, 31) if (1 << p) < rows * width] + [int(s) for s in seams]
    for c in centres:
        out += list(range(c - reach, c + reach))
    out += list(np.random.default_rng(seed).integers(0, rows, size=n_random))
    out = np.unique(np.asarray(out, dtype=np.int64))
    return out[(out >= 0) & (out < rows)]


def windows(got, idx, yardstick, scale=None):
    """Rows ``idx`` of ``got`` (rows, ...) copied to the host against ``yardstick(idx)`` (numpy float64, the same rows):
    -> max|got - ref| / scale (``scale``: max|ref| of the whole map, from the sweep; the windows' own when None)."""
    t = torch.as_tensor(np.asarray(idx, dtype=np.int64), device=got.device)
    g = got.index_select(0, t).cpu().numpy().astype(np.float64)
    r = np.asarray(yardstick(np.asarray(idx, dtype=np.int64)), dtype=np.float64).reshape(g.shape)
    assert np.all(np.isfinite(g)), "a window row is not finite"
    s = float(np.abs(r).max()) if scale is None else float(scale)
    return float(np.abs(g - r).max()) / max(s, 1e-300)


def host_rows(t, idx):
    """Rows ``idx`` of the tensor ``t`` (rows, ...) as a numpy array."""
    return t.index_select(0, torch.as_tensor(np.asarray(idx, dtype=np.int64), device=t.device)).cpu().numpy()


# ---- guarded outputs, input checksums -----------------------------------------------------------------------------------------------

class Guarded:
    """An output tensor of ``shape`` that is a view INSIDE one allocation, a band of ``BAND`` sentinel floats before and after
    it: ``view`` is pre-filled with NaN, ``check()`` asserts that both bands are untouched.  ``misalign``: floats by which the view
    is pushed off 16-byte alignment (0: aligned, so that the vector kernels stay selected -- asserted)."""

    def __init__(self, shape, device="cpu", misalign=0, dtype=torch.float32):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * BAND + 4,), SENTINEL, dtype=dtype, device=device)
        self.lo, self.hi = BAND + int(misalign), BAND + int(misalign) + n
        self.view = self.buf[self.lo:self.hi].view(shape)
        self.view.fill_(float("nan"))
        assert self.view.is_contiguous() and self.view.data_ptr() % 16 == (4 * int(misalign)) % 16, "the guarded view lost its alignment"

    def check(self, what="output"):
        before, after = self.buf[:self.lo], self.buf[self.hi:]
        nb, na = int((before != SENTINEL).sum()), int((after != SENTINEL).sum())
        assert nb == 0 and na == 0, f"{what}: {nb} floats of the band before and {na} of the band after the tensor were overwritten"


def guarded(shape, device="cpu", misalign=0):
    """-> (view, check): see ``Guarded``."""
    g = Guarded(shape, device, misalign)
    return g.view, g.check


def checksum(t, step_elems=1 << 28):
    """int64 sum of the bit patterns of a contiguous 4-byte tensor, chunked: taken before and after a call, it shows an input
    untouched without a second copy of it."""
    flat = t.reshape(-1).view(torch.int32)
    total = 0
    for r0, r1 in spans(flat.numel(), step_elems):
        total += int(flat[r0:r1].sum(dtype=torch.int64))
    return total


# ---- float64 references, plain torch -----------------------------------------------------------------------------------------------

def f64(t):
    return None if t is None else t.to(torch.float64)


def act64(v, act):
    if act == "none":
        return v
    if act == "relu":
        return torch.clamp_min(v, 0.0)
    if act == "elu":
        return torch.where(v > 0, v, torch.expm1(torch.clamp_max(v, 0.0)))
    if act == "sigmoid":
        return torch.sigmoid(v)
    if act == "tanh":
        return torch.tanh(v)
    raise ValueError(act)


def act_grad64(z, act):
    """d act / d (pre-activation) in terms of the activation's OUTPUT z."""
    if act == "none":
        return torch.ones_like(z)
    if act == "relu":
        return (z > 0).to(z.dtype)
    if act == "elu":
        return torch.where(z > 0, torch.ones_like(z), z + 1.0)
    if act == "sigmoid":
        return z * (1.0 - z)
    if act == "tanh":
        return 1.0 - z * z
    raise ValueError(act)


# batch norm: statistics over all rows (two chunked passes: the mean, then the centred squares), apply, backward
def bn_stats64(y, step):
    rows = y.shape[0]
    mean = chunked_sum(lambda a, b: f64(y[a:b]), rows, step) / rows
    var = chunked_sum(lambda a, b: (f64(y[a:b]) - mean) ** 2, rows, step) / rows
    return mean, var


def bn_apply64(y, mean, var, eps, gamma, shift, act):
    v = (f64(y) - mean) / torch.sqrt(var + eps)
    if gamma is not None:
        v = v * f64(gamma)
    if shift is not None:
        v = v + f64(shift)
    return act64(v, act)


def bn_backward_sums64(y, z, dz, mean, var, eps, act, step):
    """-> (s1 = sum g, s2 = sum g x^) with g = dz act'(z): dshift and dgamma.  ``z``: the forward's output (rows, F), or a
    function (r0, r1) -> its rows in float64."""
    rstd = 1.0 / torch.sqrt(var + eps)

    def part(a, b):
        zc = z(a, b) if callable(z) else f64(z[a:b])
        g = f64(dz[a:b]) * act_grad64(zc, act) if act != "none" else f64(dz[a:b])
        return torch.stack([g, g * (f64(y[a:b]) - mean) * rstd], dim=1)

    s = chunked_sum(part, y.shape[0], step)
    return s[0], s[1]


def bn_dy64(y, z, dz, mean, var, eps, gamma, s1, s2, rows, act):
    rstd = 1.0 / torch.sqrt(var + eps)
    g = f64(dz) * act_grad64(f64(z), act) if act != "none" else f64(dz)
    xh = (f64(y) - mean) * rstd
    k = rstd if gamma is None else f64(gamma) * rstd
    return k * (g - s1 / rows - xh * s2 / rows)


# layer norm over the trailing axis, the residual add in front
def ln_forward64(x, eps, gamma=None, beta=None, res=None):
    a = f64(x) if res is None else f64(x) + f64(res)
    mean = a.mean(dim=-1, keepdim=True)
    var = ((a - mean) ** 2).mean(dim=-1, keepdim=True)
    z = (a - mean) / torch.sqrt(var + eps)
    if gamma is not None:
        z = z * f64(gamma)
    if beta is not None:
        z = z + f64(beta)
    return z, a


def ln_backward64(a, dz, eps, gamma=None, dsum=None):
    """-> (da, dz x^, dz) of the rows given: the last two summed over ALL rows are dgamma and dbeta (``chunked_sum``)."""
    a, dz = f64(a), f64(dz)
    mean = a.mean(dim=-1, keepdim=True)
    var = ((a - mean) ** 2).mean(dim=-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (a - mean) * rstd
    g = dz if gamma is None else dz * f64(gamma)
    da = rstd * (g - g.mean(dim=-1, keepdim=True) - xh * (g * xh).mean(dim=-1, keepdim=True))
    if dsum is not None:
        da = da + f64(dsum)
    return da, dz * xh, dz


# the pseudo-convolutions' row GEMM
def patch_forward64(x, w, bias, P, act):
    z = f64(x) @ f64(w)
    if bias is not None:
        z = z + f64(bias).repeat(w.shape[1] // P)
    return act64(z, act)


def patch_dz64(y, dy, act):
    return f64(dy) * act_grad64(f64(y), act) if act != "none" else f64(dy)


# NEST pooling of (rows_out * group, F) maps
def pool_forward64(x, group, kind):
    x3 = f64(x).reshape(-1, group, x.shape[-1])
    return x3.max(dim=1).values if kind == "MAX" else x3.mean(dim=1)


def pool_backward32(x, dy, group, kind):
    """The gradient as the kernel defines it, float32 and exact: dy / group to every child (a power of four: no rounding), or dy to
    the FIRST child that holds the maximum.  ``x`` (rows_out * group, F), ``dy`` (rows_out, F) -> (rows_out * group, F)."""
    F = dy.shape[-1]
    if kind == "AVG":
        return (dy * (1.0 / group)).unsqueeze(1).expand(-1, group, -1).reshape(-1, F)
    x3 = x.reshape(-1, group, F)
    is_max = x3 == x3.max(dim=1, keepdim=True).values
    first = is_max & (torch.cumsum(is_max.to(torch.int32), dim=1) == 1)
    return torch.where(first, dy.unsqueeze(1), torch.zeros((), dtype=dy.dtype, device=dy.device)).reshape(-1, F)


def residual64(y, skip, alpha, act, act_before):
    return act64(f64(y), act) + alpha * f64(skip) if act_before else act64(f64(y) + alpha * f64(skip), act)


# one pass of an ELL table over one map: rows [r0, r1) of out = table @ x, x (M, C)
def ell_rows64(cols, vals, x, r0, r1, reps=None, pass_index=0, mask=None):
    """``dsph_ell_smooth`` and, with reps / mask None, the sparse product of ``dsph_cheb_step``: an entry outside [0, M) is an empty
    slot (weight 0).  ``reps``: int tensor [C]; ``mask``: (M, 1) or (M, C)."""
    M = x.shape[0]
    c = cols[r0:r1].to(torch.int64)
    ok = (c >= 0) & (c < M)
    w = torch.where(ok, f64(vals[r0:r1]), torch.zeros((), dtype=torch.float64, device=x.device))
    g = f64(x[torch.where(ok, c, torch.zeros_like(c))])          # (r, W, C)
    out = (g * w.unsqueeze(-1)).sum(dim=1)
    if reps is not None:
        out = torch.where((reps > pass_index).unsqueeze(0), out, f64(x[r0:r1]))
    if mask is not None:
        out = out * f64(mask[r0:r1])
    return out


def transposed_table(cols, vals):
    """The table of the transposed matrix, padded with col = row, val = 0 (``include/dsphere.h``): -> (colsT int32 [M, WT], valsT).
    Entries outside [0, M) are dropped; the entries of a row keep the order of the rows they came from."""
    M, W = cols.shape
    c = cols.reshape(-1).to(torch.int64)
    r = torch.arange(M, device=cols.device, dtype=torch.int64).repeat_interleave(W)
    keep = (c >= 0) & (c < M)
    c, r, v = c[keep], r[keep], vals.reshape(-1)[keep]
    order = torch.sort(c, stable=True).indices
    c, r, v = c[order], r[order], v[order]
    counts = torch.bincount(c, minlength=M)
    WT = max(int(counts.max()), 1)
    start = torch.cumsum(counts, 0) - counts
    slot = torch.arange(c.numel(), device=c.device) - start[c]
    colsT = torch.arange(M, device=cols.device, dtype=torch.int32).unsqueeze(1).repeat(1, WT)
    valsT = torch.zeros((M, WT), dtype=vals.dtype, device=vals.device)
    colsT[c, slot] = r.to(torch.int32)
    valsT[c, slot] = v
    return colsT, valsT


def transposed_neighbours(nbr):
    """The neighbour table of the transposed graph, -1 padded: row j lists the i whose row names j."""
    colsT, valsT = transposed_table(nbr, torch.ones(nbr.shape, dtype=torch.float32, device=nbr.device))
    return torch.where(valsT > 0, colsT, torch.full_like(colsT, -1))


# attention over a neighbour table, one map: q, k, v (M, d) (rows of any stride), nbr int32 [M, W] (-1: unused)
def _gather_heads(t, idx, heads):
    g = f64(t[idx])                                                  # (r, W, d)
    return g.reshape(g.shape[0], g.shape[1], heads, -1)


def attention_rows64(q, k, v, nbr, r0, r1, heads, dout=None):
    """Rows [r0, r1) -> (out (r, d), lse (r, heads)) and, with ``dout`` (M, d), also (delta (r, heads), dq (r, d))."""
    M, d = q.shape
    D = d // heads
    scale = 1.0 / math.sqrt(D)
    idx = nbr[r0:r1].to(torch.int64)
    ok = (idx >= 0) & (idx < M)
    safe = torch.where(ok, idx, torch.zeros_like(idx))
    q4 = f64(q[r0:r1]).reshape(-1, 1, heads, D)
    k4, v4 = _gather_heads(k, safe, heads), _gather_heads(v, safe, heads)
    s = (q4 * k4).sum(-1) * scale                                    # (r, W, heads)
    s = torch.where(ok.unsqueeze(-1), s, torch.full((), -float("inf"), dtype=torch.float64, device=s.device))
    any_ok = ok.any(dim=1).reshape(-1, 1)
    lse = torch.where(any_ok, torch.logsumexp(torch.where(any_ok.unsqueeze(-1), s, torch.zeros_like(s)), dim=1), torch.zeros((), dtype=torch.float64, device=s.device))
    p = torch.where(ok.unsqueeze(-1), torch.exp(s - lse.unsqueeze(1)), torch.zeros_like(s))
    out = (p.unsqueeze(-1) * v4).sum(dim=1)                          # (r, heads, D)
    if dout is None:
        return out.reshape(-1, d), lse
    g4 = f64(dout[r0:r1]).reshape(-1, 1, heads, D)
    delta = (g4.squeeze(1) * out).sum(-1)                            # (r, heads)
    gv = (g4 * v4).sum(-1)                                           # (r, W, heads)
    dq = ((p * (gv - delta.unsqueeze(1))).unsqueeze(-1) * k4).sum(dim=1) * scale
    return out.reshape(-1, d), lse, delta, dq.reshape(-1, d)


def attention_dkv_rows64(q, k, v, dout, lse, delta, nbrT, j0, j1, heads):
    """dk, dv of rows [j0, j1) over their in-edges (``nbrT``), from the float64 ``lse`` and ``delta`` (M, heads) of the whole map."""
    M, d = q.shape
    D = d // heads
    scale = 1.0 / math.sqrt(D)
    idx = nbrT[j0:j1].to(torch.int64)
    ok = (idx >= 0) & (idx < M)
    safe = torch.where(ok, idx, torch.zeros_like(idx))
    q4, g4 = _gather_heads(q, safe, heads), _gather_heads(dout, safe, heads)
    k4 = f64(k[j0:j1]).reshape(-1, 1, heads, D)
    v4 = f64(v[j0:j1]).reshape(-1, 1, heads, D)
    s = (q4 * k4).sum(-1) * scale
    p = torch.where(ok.unsqueeze(-1), torch.exp(s - lse[safe]), torch.zeros_like(s))
    gv = (g4 * v4).sum(-1)
    dv = (p.unsqueeze(-1) * g4).sum(dim=1)
    dk = ((p * (gv - delta[safe])).unsqueeze(-1) * q4).sum(dim=1) * scale
    return dk.reshape(-1, d), dv.reshape(-1, d)


# ---- compact copies for the window yardsticks ---------------------------------------------------------------------------------------

def compact_table(table, idx, M):
    """Rows ``idx`` of an int [M, W] table (device tensor) with every row they name, renumbered for a small host copy:
    -> (region: the rows of the big map to fetch, in order; local: int64 [len(region), W] table whose rows outside ``idx`` are
    all -1; pos: where each of ``idx`` sits in ``region``)."""
    idx = np.asarray(idx, dtype=np.int64)
    t = host_rows(table, idx).astype(np.int64)
    ok = (t >= 0) & (t < M)
    region = np.unique(np.concatenate([idx, t[ok]]))
    lut = {int(r): i for i, r in enumerate(region)}
    local = -np.ones((region.size, t.shape[1]), dtype=np.int64)
    pos = np.array([lut[int(r)] for r in idx], dtype=np.int64)
    loc = np.array([lut[int(c)] if o else -1 for c, o in zip(t.reshape(-1), ok.reshape(-1))], dtype=np.int64).reshape(t.shape)
    local[pos] = loc
    return region, local, pos
