"""GPU tests of the NEST pooling kernels (``dsph_healpix_pool`` / ``dsph_healpix_pool_backward``) and of ``HealpyPool`` on them
(``pytest -m gpu``).

Forward reference: ``np.max`` / ``np.mean`` over the 4^p children in float64 (``np.max`` propagates NaN).  The maximum selects one
of its inputs, so it is compared bit for bit; the mean to 1e-6 by helpers.rel_err.  Backward rule of the maximum, written out in ``max_backward_rule``: dy goes to the FIRST child, in
row order, that holds the output value -- a NaN child holds a NaN output -- and every other child gets exactly 0; dx is dy or 0, so
it is compared bit for bit too.  The edge cases use nside 4 or 8 and N = 2.
"""

import numpy as np
import pytest
import torch

from deepsphere import _native, healpy_layers
from helpers import offset_view, rel_err
from oracle import cheb_oracle as orc

pytestmark = pytest.mark.gpu

N = 2
POOL = {"MAX": _native.POOL_MAX, "AVG": _native.POOL_AVG}


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).cuda()


def pool_ref(x, g, pool_type):
    """float64: (N, M, F) -> (N, M / g, F)."""
    n, M, F = x.shape
    blocks = np.asarray(x, dtype=np.float64).reshape(n, M // g, g, F)
    return np.max(blocks, axis=2) if pool_type == "MAX" else np.mean(blocks, axis=2)


def max_backward_rule(x, dy, g):
    """dx of the maximum: dy to the first child (row order) that holds the output, a NaN child holding a NaN output; 0 elsewhere."""
    n, M, F = x.shape
    blocks = np.asarray(x).reshape(n, M // g, g, F)
    out = np.max(blocks, axis=2, keepdims=True)
    holds = np.where(np.isnan(out), np.isnan(blocks), blocks == out)
    assert holds.any(axis=2).all()
    first = holds.argmax(axis=2)  # (the first True)
    dx = np.zeros(blocks.shape, dtype=dy.dtype)
    np.put_along_axis(dx, first[:, :, None, :], np.asarray(dy)[:, :, None, :], axis=2)
    return dx.reshape(n, M, F)


def layer_forward_backward(x, dy, p, pool_type):
    """HealpyPool on the GPU with autograd -> (y, dx) as numpy."""
    xt = _dev(x).requires_grad_(True)
    y = healpy_layers.HealpyPool(p, pool_type)(xt)
    y.backward(_dev(dy))
    torch.cuda.synchronize()
    return y.detach().cpu().numpy(), xt.grad.cpu().numpy()


def children(x, g):
    """(N, M, F) -> a writable view (N, M / g, F, g): the last axis runs over the children of one output element."""
    n, M, F = x.shape
    return x.reshape(n, M // g, g, F).transpose(0, 1, 3, 2)


@pytest.mark.parametrize("p,F,pool_type", [(1, 16, "MAX"), (1, 16, "AVG"), (2, 5, "MAX"), (3, 7, "AVG"), (1, 64, "MAX")])
def test_nest_pooling_kernels(p, F, pool_type):
    """HealpyPool on the GPU (dsph_healpix_pool) against the oracle restatement of healpy_layers.py:20-85, bit for bit for
    the maximum, to rounding for the mean; the input gradient (dsph_healpix_pool_backward) against the host framework's
    autograd of the same reduction."""
    nside, N = 16, 3
    M = 12 * nside * nside
    rng = np.random.default_rng(p * 100 + F)
    x = rng.standard_normal((N, M, F)).astype(np.float32)
    layer = healpy_layers.HealpyPool(p, pool_type)
    xt = _dev(x).requires_grad_(True)
    y = layer(xt)
    ref = orc.healpy_pool(x.astype(np.float64), p, pool_type)
    assert y.shape == ref.shape
    if pool_type == "MAX":
        assert np.array_equal(y.detach().cpu().numpy(), ref.astype(np.float32))
    else:
        assert rel_err(y.detach().cpu().numpy(), ref) < 1e-6
    dy = rng.standard_normal(ref.shape).astype(np.float32)
    y.backward(_dev(dy))
    xr = torch.from_numpy(x).requires_grad_(True)
    g = 4 ** p
    blocks = xr.reshape(N, M // g, g, F)
    (blocks.amax(dim=2) if pool_type == "MAX" else blocks.mean(dim=2)).backward(torch.from_numpy(dy))
    assert rel_err(xt.grad.cpu().numpy(), xr.grad.numpy()) < 1e-6
    if pool_type == "MAX":  # tie-free data: the rule and autograd agree, and dx is dy or 0 exactly
        assert np.array_equal(xt.grad.cpu().numpy(), max_backward_rule(x, dy, g))
    with pytest.raises(IOError):
        layer(_dev(x[:, : M - 1]))


@pytest.mark.parametrize("F", [4, 5])  # 4: a lane loads 16 bytes; 5: one channel per lane
@pytest.mark.parametrize("p", [1, 2])
def test_ties_go_to_the_first_child(p, F):
    """What pooling sees behind a ReLU: a quarter of the groups all zero, and in another quarter the maximum repeated in a later
    child.  The maximum and its gradient bit for bit (dy to the first holder, exact zeros elsewhere), the mean to 1e-6."""
    M, g = 12 * 8 * 8, 4 ** p
    rng = np.random.default_rng(10 * p + F)
    x = np.maximum(rng.standard_normal((N, M, F)), 0).astype(np.float32)
    ch = children(x, g)
    pick = rng.random(ch.shape[:3])
    ch[pick < 0.25] = 0.0
    arg = ch.argmax(axis=3)
    later = np.minimum(arg + 1 + rng.integers(0, g, size=arg.shape) % np.maximum(g - 1 - arg, 1), g - 1)
    repeat = (pick >= 0.25) & (pick < 0.5)
    idx = np.nonzero(repeat)
    ch[idx + (later[idx],)] = ch.max(axis=3)[idx]
    tied = (ch == ch.max(axis=3, keepdims=True)).sum(axis=3) > 1
    assert (ch[pick < 0.25] == 0).all() and tied.mean() > 0.35 and not tied.all() and np.shares_memory(ch, x)
    dy = rng.standard_normal((N, M // g, F)).astype(np.float32)
    y, dx = layer_forward_backward(x, dy, p, "MAX")
    assert np.array_equal(y, pool_ref(x, g, "MAX").astype(np.float32))
    assert np.array_equal(dx, max_backward_rule(x, dy, g))
    assert (np.count_nonzero(children(dx, g), axis=3) <= 1).all()  # one child at the most receives dy
    y, dx = layer_forward_backward(x, dy, p, "AVG")
    assert rel_err(y, pool_ref(x, g, "AVG")) < 1e-6
    assert rel_err(dx, np.repeat(dy.astype(np.float64) / g, g, axis=1)) < 1e-6


@pytest.mark.parametrize("F", [4, 5])
def test_minus_infinity(F):
    """Groups of nothing but -inf give -inf and send dy to child 0; -inf beside finite children never wins."""
    p, g, M = 1, 4, 12 * 4 * 4
    rng = np.random.default_rng(20 + F)
    x = rng.standard_normal((N, M, F)).astype(np.float32)
    ch = children(x, g)
    pick = rng.random(ch.shape[:3])
    ch[pick < 0.2] = -np.inf
    some = (pick >= 0.2) & (pick < 0.6)
    ch[some & (rng.random(ch.shape[:3]) < 0.5), 0] = -np.inf      # in the first child
    ch[some, 2] = -np.inf                                          # in a middle one
    ch[some & (rng.random(ch.shape[:3]) < 0.3), 3] = -np.inf      # in the last
    assert np.isinf(ch).all(axis=3).any() and (np.isinf(ch).any(axis=3) & ~np.isinf(ch).all(axis=3)).any()
    dy = rng.standard_normal((N, M // g, F)).astype(np.float32)
    y, dx = layer_forward_backward(x, dy, p, "MAX")
    assert np.array_equal(y, pool_ref(x, g, "MAX").astype(np.float32))
    assert np.array_equal(np.isneginf(y), np.isinf(ch).all(axis=3))
    assert np.array_equal(dx, max_backward_rule(x, dy, g))
    all_inf = np.isinf(ch).all(axis=3)
    assert np.array_equal(children(dx, g)[all_inf][:, 0], dy[all_inf]) and (children(dx, g)[all_inf][:, 1:] == 0).all()


def nan_map(p, F, seed):
    """A Gaussian map with a NaN in the first, a middle or the last child of some groups, and some groups of nothing else."""
    g, M = 4 ** p, 12 * 4 * 4 if p == 1 else 12 * 8 * 8
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, M, F)).astype(np.float32)
    ch = children(x, g)
    pick = rng.random(ch.shape[:3])
    ch[pick < 0.1, 0] = np.nan
    ch[(pick >= 0.1) & (pick < 0.2), g // 2] = np.nan
    ch[(pick >= 0.2) & (pick < 0.3), g - 1] = np.nan
    ch[(pick >= 0.3) & (pick < 0.4)] = np.nan
    both = (pick >= 0.4) & (pick < 0.5)                            # two of them: the first one takes dy
    ch[both, 1] = np.nan
    ch[both, g - 1] = np.nan
    return x, g, M, rng


@pytest.mark.parametrize("p,F", [(1, 4), (2, 5), (1, 8)])
def test_max_pooling_propagates_nan(p, F):
    """A group with a NaN child pools to NaN, as ``np.max`` and the CPU branch of the same layer (``amax``) have it: a layer that
    reports an out-of-range input as non-finite rows (DSPH_PREC_F16X3) stays loud behind HealpyPool("MAX").  Everywhere else the
    GPU and CPU branches agree bit for bit."""
    x, g, M, rng = nan_map(p, F, 30 + F)
    has_nan = np.isnan(children(x, g)).any(axis=3)
    assert has_nan.any() and not has_nan.all() and np.isnan(children(x, g)).all(axis=3).any()
    layer = healpy_layers.HealpyPool(p, "MAX")
    with torch.no_grad():
        y = layer(_dev(x)).cpu().numpy()
        y_cpu = layer(torch.from_numpy(x)).numpy()
    assert np.array_equal(np.isnan(y), has_nan)
    assert np.array_equal(np.isnan(y_cpu), has_nan) and np.array_equal(y, y_cpu, equal_nan=True)
    assert np.array_equal(y, pool_ref(x, g, "MAX").astype(np.float32), equal_nan=True)


@pytest.mark.parametrize("p,F", [(1, 4), (2, 5)])
def test_max_pooling_gradient_goes_to_the_first_nan_child(p, F):
    """Through the C ABI into a dx filled with a sentinel beforehand: every element is written, dy lands on the first NaN child
    of a group that has one, on the first maximum of the others, and the rest is exactly 0.  The layer's autograd gives the same."""
    x, g, M, rng = nan_map(p, F, 40 + F)
    dy = rng.standard_normal((N, M // g, F)).astype(np.float32)
    want = max_backward_rule(x, dy, g)
    nan_child = np.isnan(children(x, g))
    first_nan = nan_child.argmax(axis=3)
    sel = nan_child.any(axis=3)
    assert np.array_equal(np.take_along_axis(children(want, g), first_nan[..., None], axis=3)[..., 0][sel], dy[sel])
    xd, dyd = _dev(x), _dev(dy)
    sentinel = 12345.0
    dx = torch.full((N, M, F), sentinel, dtype=torch.float32, device="cuda")
    rc = _native.lib().dsph_healpix_pool_backward(_native._ptr(xd), _native._ptr(dyd), _native._ptr(dx), N, M // g, F, g, _native.POOL_MAX, 0,
                                                  _native._stream_ptr(xd.device))
    torch.cuda.synchronize()
    got = dx.cpu().numpy()
    assert rc == 0 and not (got == sentinel).any() and not np.isnan(got).any()
    assert np.array_equal(got, want)
    _, dx_layer = layer_forward_backward(x, dy, p, "MAX")
    assert np.array_equal(dx_layer, want)


@pytest.mark.parametrize("p,F", [(1, 4), (2, 5)])
def test_average_pooling_propagates_nan(p, F):
    x, g, M, _ = nan_map(p, F, 50 + F)
    has_nan = np.isnan(children(x, g)).any(axis=3)
    layer = healpy_layers.HealpyPool(p, "AVG")
    with torch.no_grad():
        y = layer(_dev(x)).cpu().numpy()
        y_cpu = layer(torch.from_numpy(x)).numpy()
    assert np.array_equal(np.isnan(y), has_nan) and np.array_equal(np.isnan(y_cpu), has_nan)
    assert rel_err(y[~has_nan], pool_ref(x, g, "AVG")[~has_nan]) < 1e-6


@pytest.mark.parametrize("pool_type", ["MAX", "AVG"])
def test_a_misaligned_map_takes_the_scalar_kernel_and_gives_the_same_bits(pool_type):
    """F % 4 == 0 but x four bytes off 16-byte alignment: one channel per lane instead of four, the same sums in the same order."""
    g, M, F = 4, 12 * 4 * 4, 8
    x = np.random.default_rng(60).standard_normal((N, M, F)).astype(np.float32)
    view = offset_view(x, 1)
    assert view.data_ptr() % 16 == 4
    aligned = _dev(x)
    assert aligned.data_ptr() % 16 == 0
    y_view, y_aligned = _native.healpix_pool(view, g, POOL[pool_type]), _native.healpix_pool(aligned, g, POOL[pool_type])
    torch.cuda.synchronize()
    assert torch.equal(y_view, y_aligned)
    ref = pool_ref(x, g, pool_type)
    assert np.array_equal(y_view.cpu().numpy(), ref.astype(np.float32)) if pool_type == "MAX" else rel_err(y_view.cpu().numpy(), ref) < 1e-6


@pytest.mark.parametrize("group", [64, 256])
def test_long_groups_and_a_single_output_row_through_the_c_abi(group):
    """Groups of 4^3 and 4^4 children, three channels, one output row per map; the mean to the module's 1e-6."""
    F, rows_out = 3, 1
    rng = np.random.default_rng(group)
    x = rng.standard_normal((N, rows_out * group, F)).astype(np.float32)
    dy = rng.standard_normal((N, rows_out, F)).astype(np.float32)
    xd, dyd = _dev(x), _dev(dy)
    L, p, stream = _native.lib(), _native._ptr, _native._stream_ptr(xd.device)
    for pool_type in ("MAX", "AVG"):
        y = torch.full((N, rows_out, F), 7.0, dtype=torch.float32, device="cuda")
        dx = torch.full((N, rows_out * group, F), 7.0, dtype=torch.float32, device="cuda")
        assert L.dsph_healpix_pool(p(xd), p(y), N, rows_out, F, group, POOL[pool_type], 0, stream) == 0
        assert L.dsph_healpix_pool_backward(p(xd), p(dyd), p(dx), N, rows_out, F, group, POOL[pool_type], 0, stream) == 0
        torch.cuda.synchronize()
        ref = pool_ref(x, group, pool_type)
        if pool_type == "MAX":
            assert np.array_equal(y.cpu().numpy(), ref.astype(np.float32))
            assert np.array_equal(dx.cpu().numpy(), max_backward_rule(x, dy, group))
        else:
            err = rel_err(y.cpu().numpy(), ref)
            print(f"group {group}: mean rel_err {err:.3e}")
            assert err < 1e-6
            want = np.repeat(dy * np.float32(1.0 / group), group, axis=1)  # dy times the fp32 reciprocal, one rounding
            assert np.abs(dx.cpu().numpy() - want.astype(np.float64)).max() <= 2.0**-24 * np.abs(want).max()
