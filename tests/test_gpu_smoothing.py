"""GPU tests of the smoothing kernel (``dsph_ell_smooth``) and of ``HealpySmoothing`` on it (``pytest -m gpu``).

Reference: tests/smoothing_ref.py, the passes restated in float64 ON THE SAME fp32 TABLE, so only the kernel's arithmetic is
compared.  The tolerance is derived, not measured.  One pass computes, per output, a chain of fused multiply-adds in every lane
and a butterfly over the lanes: at most W + log2(64) <= W + 8 roundings of 2^-24 relative to the running magnitude.  The weights
are nonnegative and sum to 1, so no partial sum exceeds max|x|; the fp32 row sum is itself off 1 by up to the same amount
(factor 2); r passes add up:
    |err| <= 2 r (W + 8) 2^-24 max|x|.
The input gradient is the same passes on the transposed table: its width WT takes the place of W, and a pass can scale a map by
S = max_m sum_j k[j, m] (the largest column sum, in place of the row sum 1), so max|g| S^r takes the place of max|x|.
N = 2 throughout; full sky at nside 16 (3,072 pixels) and a cap of 260 pixels at nside 8.
"""

import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

import smoothing_ref as ref
from deepsphere import _native, healpix
from deepsphere.healpy_layers import HealpyChebyshev, HealpySmoothing
from deepsphere.healpy_networks import HealpyGCNN

pytestmark = pytest.mark.gpu

N = 2
# sigma in units of the pixel resolution sqrt(4 pi / npix); the table widths the factors give are asserted in the first test
TABLES = {"w9": (16, None, 0.5), "w30": (16, None, 1.0), "w178": (16, None, 2.5), "w542": (16, None, 4.5), "cap": (8, "cap", 1.0)}


@functools.lru_cache(maxsize=None)
def base_layer(name):
    nside, patch, factor = TABLES[name]
    indices = healpix.cap_indices(8) if patch == "cap" else np.arange(12 * nside * nside)
    return HealpySmoothing(nside, indices, sigma=factor * np.sqrt(4 * np.pi / (12 * nside * nside)), arcmin=False)


def variant(name, reps=None, mask=None):
    """A layer on the cached table of ``name`` with its own repetitions and mask."""
    layer = copy.copy(base_layer(name))
    layer.per_channel_repetitions = None if reps is None else np.array(reps)
    layer.mask, layer.n_channels, layer._dev, layer._tables_T = mask, None, {}, None
    return layer


@functools.lru_cache(maxsize=None)
def table(name):
    layer = base_layer(name)
    return layer.cols.cpu().numpy(), layer.vals.cpu().numpy()


@functools.lru_cache(maxsize=None)
def maps(M, C, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, M, C)).astype(np.float32), rng.standard_normal((N, M, C)).astype(np.float32)


def bound(W, r, scale):
    return 2 * r * (W + 8) * 2.0**-24 * scale


def run(layer, x):
    y = layer(torch.as_tensor(x).cuda())
    torch.cuda.synchronize()
    return y.cpu().numpy()


def test_tables_are_the_classes_the_cases_name():
    W = {name: table(name)[0].shape[1] for name in TABLES}
    print(W)
    assert W["w9"] < 16               # fewer entries than lanes in a group
    assert 16 < W["w30"] <= 128       # 16-lane groups, several entries per lane
    assert 128 < W["w178"] <= 512     # 64-lane groups
    assert W["w542"] > 512            # more than 8 entries per lane of a 64-lane group: a second chunk
    assert table("cap")[0].shape[0] == 260 and 16 < W["cap"] <= 128


@pytest.mark.parametrize("C", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("name", list(TABLES))
def test_forward_parity(name, C):
    cols, vals = table(name)
    x, _ = maps(cols.shape[0], C)
    got = run(variant(name), x)
    err = np.abs(got - ref.apply(cols, vals, x)).max()
    tol = bound(cols.shape[1], 1, np.abs(x).max())
    print(f"{name} C {C}: err {err:.3e} bound {tol:.3e}")
    assert got.dtype == np.float32 and got.shape == x.shape and err <= tol


@pytest.mark.parametrize("C", [6, 8])
def test_channel_counts_of_several_vectors(C):
    cols, vals = table("w30")
    x, _ = maps(cols.shape[0], C)
    err = np.abs(run(variant("w30"), x) - ref.apply(cols, vals, x)).max()
    assert err <= bound(cols.shape[1], 1, np.abs(x).max())


@pytest.mark.parametrize("mask_shape", ["M", "MC"])
def test_repetitions_and_masks(mask_shape):
    cols, vals = table("w30")
    M, C, reps = cols.shape[0], 4, [0, 1, 3, 2]
    x, _ = maps(M, C)
    mask = np.random.default_rng(3).random((M,) if mask_shape == "M" else (M, C)) < 0.7
    got = run(variant("w30", reps=reps, mask=mask), x)
    err = np.abs(got - ref.apply(cols, vals, x, reps, mask)).max()
    tol = bound(cols.shape[1], 3, np.abs(x).max())
    print(f"mask {mask_shape}: err {err:.3e} bound {tol:.3e}")
    assert err <= tol
    m0 = (mask if mask.ndim == 1 else mask[:, 0]).astype(np.float32)
    assert np.array_equal(got[:, :, 0], x[:, :, 0] * m0[None])  # the channel no pass touches: bit for bit x times the mask
    assert (got[:, ~m0.astype(bool), 0] == 0).all()


def test_no_repetition_at_all_runs_no_pass():
    M = table("w30")[0].shape[0]
    x, _ = maps(M, 2)
    assert np.array_equal(run(variant("w30", reps=[0, 0]), x), x)
    mask = np.random.default_rng(4).random(M) < 0.5
    assert np.array_equal(run(variant("w30", reps=[0, 0], mask=mask), x), x * mask[None, :, None].astype(np.float32))


def test_constant_map_stays_constant_and_runs_repeat_bitwise():
    for name in ("w30", "w178", "w542"):
        cols, _ = table(name)
        const = np.full((N, cols.shape[0], 3), 1.7, dtype=np.float32)
        assert np.abs(run(variant(name), const) - np.float32(1.7)).max() <= bound(cols.shape[1], 1, 1.7)
        x, _ = maps(cols.shape[0], 3)
        layer = variant(name, reps=[2, 1, 2])
        assert np.array_equal(run(layer, x), run(layer, x))


@pytest.mark.parametrize("name,C,reps,masked", [("w30", 4, [0, 1, 3, 2], True), ("w178", 1, None, False), ("cap", 2, [2, 1], True),
                                                ("w9", 3, None, False)])
def test_backward(name, C, reps, masked):
    cols, vals = table(name)
    M = cols.shape[0]
    x, g = maps(M, C)
    mask = (np.random.default_rng(5).random((M, C)) < 0.7) if masked else None
    layer = variant(name, reps=reps, mask=mask)
    xt = torch.as_tensor(x).cuda().requires_grad_(True)
    gt = torch.as_tensor(g).cuda()
    layer(xt).backward(gt)
    torch.cuda.synchronize()
    dx = xt.grad.cpu().numpy()
    K = ref.dense(cols, vals)
    want = ref.apply_transposed(K, g, reps, mask)
    WT, S, r = layer._tables_T[0].shape[1], K.sum(axis=0).max(), ref.n_passes(reps)
    err, tol = np.abs(dx - want).max(), bound(WT, r, np.abs(g).max() * max(S, 1.0) ** r)
    print(f"{name} C {C} reps {reps}: WT {WT} S {S:.3f} err {err:.3e} bound {tol:.3e}")
    assert WT >= cols.shape[1] and err <= tol
    # deterministic
    xt.grad = None
    layer(xt).backward(gt)
    assert torch.equal(xt.grad.cpu(), torch.as_tensor(dx))


def test_no_transposed_table_without_a_gradient():
    layer = variant("w30")
    x, _ = maps(table("w30")[0].shape[0], 2)
    y = layer(torch.as_tensor(x).cuda())
    assert not y.requires_grad and layer._tables_T is None
    with torch.no_grad():
        layer(torch.as_tensor(x).cuda().requires_grad_(True))
    assert layer._tables_T is None


def test_c_abi_refuses_bad_arguments_before_any_launch():
    layer = base_layer("w9")
    cols, vals = layer._tables(torch.device("cuda", 0))
    M, W = cols.shape
    C = 2
    x = torch.as_tensor(maps(M, C)[0]).cuda()
    y = torch.full_like(x, 7.0)
    mask = torch.ones((M, 3), device="cuda")
    stream = _native._stream_ptr(x.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(xp, yp, width, mask_ptr, mask_C):
        return _native.lib().dsph_ell_smooth(p(cols), p(vals), M, width, xp, yp, N, C, None, 0, mask_ptr, mask_C, 0, stream)

    before = x.clone()
    assert call(p(x), p(x), W, None, 1) == -1 and "overlap" in _native.last_error()          # x is y
    shifted = ctypes.c_void_p(x.data_ptr() + 4 * C)                                            # y inside x
    assert call(p(x), shifted, W, None, 1) == -1 and "overlap" in _native.last_error()
    assert call(p(x), p(y), 0, None, 1) == -1 and "W" in _native.last_error()
    assert call(p(x), p(y), -3, None, 1) == -1
    assert call(p(x), p(y), W, p(mask), 3) == -1 and "mask_C" in _native.last_error()
    torch.cuda.synchronize()
    assert torch.equal(x, before) and bool((y == 7.0).all())                                    # nothing ran
    with pytest.raises(ValueError, match="overlap"):
        _native.ell_smooth(cols, vals, x, out=x)
    assert call(p(x), p(y), W, None, 1) == 0                                                   # and the good call does run
    torch.cuda.synchronize()
    assert bool((y != 7.0).all())


def test_in_a_network():
    idx = np.arange(12 * 16 * 16)
    smooth = variant("w30")
    model = HealpyGCNN(16, idx, [smooth, HealpyChebyshev(K=3, Fout=4)])
    x = torch.as_tensor(maps(len(idx), 2)[0]).cuda()
    with torch.no_grad():
        whole = model(x)
        parts = model[1](smooth(x))
    torch.cuda.synchronize()
    assert tuple(whole.shape) == (N, len(idx), 4) and torch.equal(whole, parts)
