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

The real tables reach four of the kernel's classes.  A launch picks G = 16 lanes per row for W <= 128 and 64 above, E = min(8,
ceil(W / G)) entries per lane and chunk, and VEC = 4, 2 or 1 channels per access from C and the alignment of the maps: 14
reachable (G, E) classes (G = 64 needs W > 128, so E >= 3 there) times three widths.  The synthetic tables below (M = 37: a
multiple of neither 16 nor 4 rows per workgroup, more than one workgroup for both G) call ``_native.ell_smooth`` at both ends of
every class and at every width, against ``smoothing_ref.apply_pass`` and the same bound with r = 1.  Where a mask is not 0 / 1 its
multiply is one more rounding, inside the bound's slack: the bound counts W roundings of the sum, the kernel's longest chain is
8 multiply-adds, 6 butterfly steps and one add per chunk.
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
from helpers import offset_view

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


# ---- synthetic tables: every (G, E) class at both ends, every vector width -------------------------------------------------

SYN_M = 37
G16_WIDTHS = [1, 15, 16, 17, 48, 49, 80, 96, 112, 113, 128]           # E = 1, 1, 1, 2, 3, 4, 5, 6, 7, 8, 8
G64_WIDTHS = [129, 192, 193, 257, 321, 385, 449, 512, 513, 1024, 1025]  # E = 3, 3, 4, 5, 6, 7, 8, 8, then 2, 2 and 3 chunks of 8
# (C, offset of the maps in floats) -> the vector width the launch takes
VEC_CASES = {(8, 0): 4, (4, 0): 4, (6, 0): 2, (4, 2): 2, (4, 1): 1, (6, 1): 1, (3, 0): 1}
OUT_OF_RANGE = [-1, SYN_M, SYN_M + 5, 2**31 - 1]


def group_and_entries(W):
    G = 16 if W <= 128 else 64
    return G, min(8, -(-W // G))


@functools.lru_cache(maxsize=None)
def synthetic_table(W, empty_slots=False, seed=0):
    """-> (cols int32 [M, W], vals float32 [M, W]): columns uniform in [0, M) (duplicates allowed, W may exceed M), weights
    nonnegative, every row summing to 1 over its valid entries.  ``empty_slots``: a random third of the entries, anywhere in the
    row, named -1, M, M + 5 or 2^31 - 1 (their weights stay, and must not count), and row 11 made of nothing else."""
    rng = np.random.default_rng(1000 * seed + W)
    cols = rng.integers(0, SYN_M, size=(SYN_M, W)).astype(np.int32)
    vals = rng.random((SYN_M, W)) + 1e-3
    ok = np.ones((SYN_M, W), dtype=bool)
    if empty_slots:
        ok = rng.random((SYN_M, W)) >= 1 / 3
        ok[11] = False
        ok[12, 1:] = False                                            # and a row with one valid entry, in the first slot
        ok[12, 0] = True
        cols[~ok] = rng.choice(np.array(OUT_OF_RANGE, dtype=np.int32), size=int((~ok).sum()))
    norm = np.where(ok, vals, 0.0).sum(axis=1, keepdims=True)
    vals = (vals / np.where(norm > 0, norm, 1.0)).astype(np.float32)
    return cols, vals


@functools.lru_cache(maxsize=None)
def synthetic_map(C):
    return np.random.default_rng(40 + C).standard_normal((N, SYN_M, C)).astype(np.float32)


def vector_width(x, y, C):
    """The width the launch must take, INFERRED from the pointers and C by the launcher's documented rule: the kernel offers no
    way to observe it.  What carries weight is the alignment asserted in ``helpers.offset_view`` and the bit-for-bit equality of
    runs that differ in nothing else."""
    al = x.data_ptr() | y.data_ptr()
    return 4 if C % 4 == 0 and al % 16 == 0 else 2 if C % 2 == 0 and al % 8 == 0 else 1


def smooth_once(cols, vals, x, offset=0, reps=None, pass_index=0, mask=None):
    """One ``_native.ell_smooth`` call on maps ``offset`` floats off 16-byte alignment -> (numpy result, inferred vector width)."""
    C = x.shape[2]
    xd, yd = offset_view(x, offset), offset_view(np.full(x.shape, 7.0), offset)
    dev = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).cuda()
    out = _native.ell_smooth(dev(cols, np.int32), dev(vals, np.float32), xd, out=yd, reps=dev(reps, np.int32), pass_index=pass_index,
                             mask=dev(mask, np.float32))
    torch.cuda.synchronize()
    assert out is yd
    return yd.cpu().numpy(), vector_width(xd, yd, C)


def test_synthetic_widths_reach_every_class():
    assert [group_and_entries(W) for W in G16_WIDTHS] == [(16, e) for e in (1, 1, 1, 2, 3, 4, 5, 6, 7, 8, 8)]
    assert [group_and_entries(W) for W in G64_WIDTHS] == [(64, e) for e in (3, 3, 4, 5, 6, 7, 8, 8, 8, 8, 8)]
    assert {group_and_entries(W) for W in range(1, 4097)} == {group_and_entries(W) for W in G16_WIDTHS + G64_WIDTHS}  # all 14
    assert [-(-W // 512) for W in (512, 513, 1024, 1025)] == [1, 2, 2, 3]  # chunks of 8 entries per lane
    assert SYN_M % 16 != 0 and SYN_M % 4 != 0 and SYN_M > 16
    assert sorted(set(VEC_CASES.values())) == [1, 2, 4]


@pytest.mark.parametrize("W", G16_WIDTHS + G64_WIDTHS)
def test_every_group_entry_and_vector_class(W):
    """One (G, E) class per width, all three vector widths in it: 16-byte aligned maps of 8, 4, 6 and 3 channels, 4 channels 8
    bytes off, 4 and 6 channels 4 bytes off.  Every result against the float64 pass within the derived bound; runs that differ
    only in the vector width give the same bits (the per-lane multiply-add chain and the butterfly do not depend on it)."""
    cols, vals = synthetic_table(W)
    assert np.abs(vals.astype(np.float64).sum(axis=1) - 1).max() <= (W + 8) * 2.0**-24 and (vals >= 0).all()
    got = {}
    for (C, offset), vec in VEC_CASES.items():
        x = synthetic_map(C)
        y, took = smooth_once(cols, vals, x, offset)
        err, tol = np.abs(y - ref.apply_pass(cols, vals, x)).max(), bound(W, 1, np.abs(x).max())
        print(f"W {W} (G, E) {group_and_entries(W)} C {C} offset {offset} VEC {took}: err {err:.3e} bound {tol:.3e}")
        assert took == vec and err <= tol
        got[C, offset] = y
    assert np.array_equal(got[4, 0], got[4, 2]) and np.array_equal(got[4, 0], got[4, 1])  # VEC 4, 2, 1
    assert np.array_equal(got[6, 0], got[6, 1])                                           # VEC 2, 1


@pytest.mark.parametrize("C", [4, 3])
@pytest.mark.parametrize("W", [49, 513])
def test_empty_slots_anywhere_in_a_row(W, C):
    """A third of the entries outside [0, M), scattered through the rows with their weights left in place: they count as
    weight 0 (and are not followed: 2^31 - 1 rows of C floats would be far outside the map).  A row of nothing else is exactly 0."""
    cols, vals = synthetic_table(W, empty_slots=True)
    bad = (cols < 0) | (cols >= SYN_M)
    assert 0.25 < bad.mean() < 0.42 and bad[11].all() and bad[:, 0].any() and bad[:, W // 2].any() and not bad[:, -1].all()
    assert all((cols == v).any() for v in OUT_OF_RANGE) and (vals[bad] > 0).all()
    x = synthetic_map(C)
    y, _ = smooth_once(cols, vals, x)
    err, tol = np.abs(y - ref.apply_pass(cols, vals, x)).max(), bound(W, 1, np.abs(x).max())
    print(f"W {W} C {C}: err {err:.3e} bound {tol:.3e}")
    assert err <= tol
    assert (y[:, 11] == 0).all()
    assert np.abs(y[:, 12] - x[:, cols[12, 0]]).max() <= tol  # one valid entry of weight 1


@pytest.mark.parametrize("offset", [0, 1], ids=["VEC 4", "VEC 1"])
@pytest.mark.parametrize("mask_shape", ["M1", "MC"])
@pytest.mark.parametrize("W", [513, 1025])
def test_chunked_rows_with_repetitions_and_masks(W, mask_shape, offset):
    """More than one chunk (W > 512) together with per-channel repetitions and a mask: a later chunk adds to what the one before
    stored only for the smoothed channels, the passed-through ones are selected from x in every chunk, the mask multiplies once,
    in the last.  Smoothed channels within the bound, passed-through channels x times the mask bit for bit.  The mask holds
    zeros and fractions: a 0 / 1 mask would not notice being applied twice."""
    C, reps = 4, [0, 1, 3, 2]
    cols, vals = synthetic_table(W)
    x = synthetic_map(C)
    rng = np.random.default_rng(6)
    mask = (rng.random((SYN_M, 1 if mask_shape == "M1" else C)) * (rng.random((SYN_M, 1 if mask_shape == "M1" else C)) < 0.7)).astype(np.float32)
    assert (mask == 0).any() and ((mask > 0) & (mask < 1)).any()
    tol = bound(W, 1, np.abs(x).max())
    for pass_index in range(3):
        y, took = smooth_once(cols, vals, x, offset, reps=reps, pass_index=pass_index, mask=mask)
        want = ref.apply_pass(cols, vals, x, reps, pass_index, mask)
        smoothed = [c for c in range(C) if reps[c] > pass_index]
        kept = [c for c in range(C) if reps[c] <= pass_index]
        err = np.abs(y[..., smoothed] - want[..., smoothed]).max()
        print(f"W {W} mask {mask_shape} VEC {took} pass {pass_index}: smoothed {smoothed} err {err:.3e} bound {tol:.3e}")
        assert took == (4 if offset == 0 else 1) and smoothed and kept and err <= tol
        for c in kept:
            assert np.array_equal(y[..., c], x[..., c] * mask[None, :, c % mask.shape[1]])
    # without a mask the passed-through channels are x itself
    y, _ = smooth_once(cols, vals, x, offset, reps=reps, pass_index=1)
    assert np.array_equal(y[..., :2], x[..., :2]) and np.abs(y - ref.apply_pass(cols, vals, x, reps, 1)).max() <= tol


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
