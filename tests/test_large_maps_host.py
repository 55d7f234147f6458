"""CPU tests of the large-map checker (tests/large_map_ref.py): every planted fault is reported, a correct result passes, the
torch-float64 references equal the suite's numpy yardsticks to 1e-12 on small shapes, and the size limits that the entry points
refuse before their first HIP call are refused with the documented code and message."""

import numpy as np
import pytest
import torch

import attention_ref
import batchnorm_ref
import large_map_ref as lm
import layernorm_ref
import pseudoconv_ref
import smoothing_ref
from deepsphere import _native
from helpers import rel_err

EXACT = 1e-12
ROWS, F, STEP = 1003, 12, 64          # an odd row count, a ragged last chunk
SEAMS = (250, 501, 752)               # "documented" work-split seams of the planted-fault maps


def _map(seed=0, rows=ROWS, width=F):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((rows, width)).astype(np.float32))


def _ref_fn(x):
    """The operation of the planted-fault tests: z = tanh(x) * 3 + 1 per element, in float64."""
    return lambda a, b: torch.tanh(x[a:b].to(torch.float64)) * 3.0 + 1.0


def _correct(x):
    out, check = lm.guarded(x.shape)
    out.copy_((torch.tanh(x.to(torch.float64)) * 3.0 + 1.0).to(torch.float32))
    return out, check


def _yardstick(x):
    xn = x.numpy().astype(np.float64)
    return lambda idx: np.tanh(xn[idx]) * 3.0 + 1.0


# ---- the checker reports what it must ----------------------------------------------------------------------------------------------

def test_correct_result_passes():
    x = _map()
    before = lm.checksum(x)
    out, check = _correct(x)
    err, scale = lm.sweep(out, _ref_fn(x), STEP)
    idx = lm.window_rows(ROWS, F, seams=SEAMS)
    assert err / scale < 2e-7 and lm.windows(out, idx, _yardstick(x), scale) < 2e-7
    check()
    assert lm.checksum(x) == before
    assert lm.equal_sweep(out, lambda a, b: out[a:b].clone(), STEP) == 0


def test_wrapped_offset_is_reported():
    """Rows from R0 on repeat the rows from 0: what a kernel whose offset wraps writes."""
    x = _map()
    out, _ = _correct(x)
    R0 = 640
    out[R0:] = out[:ROWS - R0].clone()
    err, scale = lm.sweep(out, _ref_fn(x), STEP)
    assert err / scale > 0.1
    assert lm.windows(out, lm.window_rows(ROWS, F, seams=SEAMS), _yardstick(x), scale) > 0.1  # (the last rows are a window)
    assert lm.equal_sweep(out, lambda a, b: (torch.tanh(x[a:b].to(torch.float64)) * 3.0 + 1.0).to(torch.float32), STEP) >= (ROWS - R0) * F // 2


def test_unwritten_block_is_reported():
    x = _map()
    out, _ = _correct(x)
    out[300:364] = float("nan")  # the pre-fill a dropped trip of a grid-stride loop leaves
    with pytest.raises(AssertionError, match="row 300 still holds its NaN pre-fill"):
        lm.sweep(out, _ref_fn(x), STEP)
    with pytest.raises(AssertionError, match="NaN pre-fill"):
        lm.equal_sweep(out, lambda a, b: out[a:b], STEP)
    out2, _ = _correct(x)
    out2[5, 3] = float("inf")
    with pytest.raises(AssertionError, match="row 5 is not finite"):
        lm.sweep(out2, _ref_fn(x), STEP)


def test_one_wrong_row_next_to_a_seam_is_reported():
    x = _map()
    out, _ = _correct(x)
    _, scale = lm.sweep(out, _ref_fn(x), STEP)
    out[SEAMS[1] - 1] += 1e-3 * scale
    err, scale2 = lm.sweep(out, _ref_fn(x), STEP)
    assert 0.9e-3 < err / scale2 < 1.1e-3
    idx = lm.window_rows(ROWS, F, seams=SEAMS)
    assert SEAMS[1] - 1 in idx and SEAMS[1] in idx
    assert lm.windows(out, idx, _yardstick(x), scale2) > 0.9e-3


def test_changed_sentinel_is_reported():
    for where in (-1, 0):
        g = lm.Guarded((ROWS, F))
        g.check()
        assert g.view.data_ptr() % 16 == 0 and bool(torch.isnan(g.view).all())
        g.buf[g.lo - 1 if where < 0 else g.hi] = 0.0
        with pytest.raises(AssertionError, match="were overwritten"):
            g.check()
    g = lm.Guarded((7, 3), misalign=1)
    assert g.view.data_ptr() % 16 == 4
    g.view.zero_()
    g.check()


def test_checksum_sees_one_changed_bit():
    x = _map()
    before = lm.checksum(x, step_elems=1000)
    assert before == lm.checksum(x)
    x.view(torch.int32)[777, 5] ^= 1
    assert lm.checksum(x, step_elems=1000) != before


def test_window_rows_cover_the_named_places():
    rows, width = (1 << 25) + (1 << 16) + 3, 64
    idx = lm.window_rows(rows, width, seams=(12345, rows // 2))
    for c in [0, 3, rows - 1, rows - 4, (1 << 29) // 64, (1 << 30) // 64 - 1, (1 << 31) // 64, (1 << 31) // 64 - 2, 12344, 12345, rows // 2 - 1]:
        assert c in idx
    assert idx.min() >= 0 and idx.max() == rows - 1 and idx.size >= 32 + 8
    small = lm.window_rows(100, 5)
    assert small.max() == 99 and (1 << 29) // 5 not in small


# ---- the torch-float64 references against the numpy yardsticks -----------------------------------------------------------------------

@pytest.mark.parametrize("act", lm.ACTS)
def test_batch_norm_references(act):
    rng = np.random.default_rng(3)
    rows, F_, eps = 203, 7, 1e-5
    y = (rng.standard_normal((rows, F_)) * 2 + 10).astype(np.float32)
    dz = rng.standard_normal((rows, F_)).astype(np.float32)
    gamma, shift = (1 + 0.2 * rng.standard_normal(F_)).astype(np.float32), rng.standard_normal(F_).astype(np.float32)
    mean, var, z = batchnorm_ref.bn_forward(y, eps, gamma, shift, act)
    dy, dgamma, dshift = batchnorm_ref.bn_backward(y, dz, eps, gamma, shift, act)
    ty, tdz, tg, ts = (torch.from_numpy(a) for a in (y, dz, gamma, shift))
    m64, v64 = lm.bn_stats64(ty, 50)
    z64 = lm.bn_apply64(ty, m64, v64, eps, tg, ts, act)
    s1, s2 = lm.bn_backward_sums64(ty, z64, tdz, m64, v64, eps, act, 50)
    dy64 = lm.bn_dy64(ty, z64, tdz, m64, v64, eps, tg, s1, s2, rows, act)
    for got, want in ((m64, mean), (v64, var), (z64, z), (s1, dshift), (s2, dgamma), (dy64, dy)):
        assert rel_err(got.numpy(), want) < EXACT


def test_layer_norm_references():
    x, res, dz, dsum, gamma, beta = layernorm_ref.make_data(37, 24)
    z, a = layernorm_ref.ln_forward(x, 1e-3, gamma, beta, res)
    da, dgamma, dbeta = layernorm_ref.ln_backward(a, dz, 1e-3, gamma, dsum)
    t = [torch.from_numpy(v) for v in (x, res, dz, dsum, gamma, beta)]
    z64, a64 = lm.ln_forward64(t[0], 1e-3, t[4], t[5], t[1])
    da64 = lm.ln_backward64(a64, t[2], 1e-3, t[4], t[3])[0]
    sums = lm.chunked_sum(lambda r0, r1: torch.stack(lm.ln_backward64(a64[r0:r1], t[2][r0:r1], 1e-3, t[4])[1:], dim=1), 37, 10)
    for got, want in ((z64, z), (a64, a), (da64, da), (sums[0], dgamma), (sums[1], dbeta)):
        assert rel_err(got.numpy(), want) < EXACT


@pytest.mark.parametrize("act", ["none", "relu", "tanh"])
def test_patch_gemm_references(act):
    X, W, b, dY = pseudoconv_ref.make_data(53, 20, 12, 4, seed=2)
    tX, tW, tb, tdY = (torch.from_numpy(np.asarray(a, dtype=np.float32)) for a in (X, W, b, dY))
    Y = pseudoconv_ref.patch_forward(tX.numpy(), tW.numpy(), tb.numpy(), 4, act)
    assert rel_err(lm.patch_forward64(tX, tW, tb, 4, act).numpy(), Y) < EXACT
    Y32 = torch.from_numpy(Y.astype(np.float32))  # the stored output, as the epilogue's backward reads it
    dz64 = lm.patch_dz64(Y32, tdY, act)
    db64 = lm.chunked_sum(lambda r0, r1: dz64[r0:r1].reshape(r1 - r0, 3, 4).sum(dim=1), 53, 16)
    assert rel_err(db64.numpy(), pseudoconv_ref.patch_backward(tX.numpy(), tW.numpy(), Y32.numpy(), tdY.numpy(), 4, act)[2]) < EXACT


def test_pool_and_residual_references():
    rng = np.random.default_rng(5)
    x = rng.permutation(16 * 6 * 5).astype(np.float32).reshape(16 * 6, 5) / 7  # distinct values: MAX has no ties
    dy = rng.standard_normal((6, 5)).astype(np.float32)
    tx, tdy = torch.from_numpy(x), torch.from_numpy(dy)
    x3 = x.reshape(6, 16, 5).astype(np.float64)
    assert rel_err(lm.pool_forward64(tx, 16, "MAX").numpy(), x3.max(axis=1)) == 0 and rel_err(lm.pool_forward64(tx, 16, "AVG").numpy(), x3.mean(axis=1)) < EXACT
    want = np.where(x3 == x3.max(axis=1, keepdims=True), dy[:, None, :], 0.0).reshape(-1, 5)
    assert np.array_equal(lm.pool_backward32(tx, tdy, 16, "MAX").numpy(), want.astype(np.float32))
    assert np.array_equal(lm.pool_backward32(tx, tdy, 16, "AVG").numpy(), np.repeat(dy / np.float32(16), 16, axis=0))
    tied = torch.tensor([[1.0], [3.0], [3.0], [2.0]])  # a tie: the FIRST child that holds the maximum
    assert lm.pool_backward32(tied, torch.tensor([[5.0]]), 4, "MAX").reshape(-1).tolist() == [0.0, 5.0, 0.0, 0.0]
    a, b = rng.standard_normal(50).astype(np.float32), rng.standard_normal(50).astype(np.float32)
    for before in (False, True):
        want = np.tanh(a.astype(np.float64)) + 0.25 * b if before else np.tanh(a.astype(np.float64) + 0.25 * b)
        assert rel_err(lm.residual64(torch.from_numpy(a), torch.from_numpy(b), 0.25, "tanh", before).numpy(), want) < EXACT


def _table(M, W, seed, empty=True):
    rng = np.random.default_rng(seed)
    cols = rng.integers(0, M, size=(M, W)).astype(np.int32)
    vals = rng.random((M, W)).astype(np.float32)
    if empty:
        cols[rng.random((M, W)) < 0.25] = -1
        cols[3] = -1
    return cols, vals


def test_ell_references_and_transposed_table():
    M, W, C = 41, 7, 6
    cols, vals = _table(M, W, 1)
    rng = np.random.default_rng(2)
    x = rng.standard_normal((M, C)).astype(np.float32)
    reps, mask = np.array([0, 1, 2, 1, 0, 3]), rng.random((M, 1)).astype(np.float32)
    tc, tv, tx = torch.from_numpy(cols), torch.from_numpy(vals), torch.from_numpy(x)
    for r, m, p in ((None, None, 0), (reps, mask, 0), (reps, None, 1)):
        want = smoothing_ref.apply_pass(cols, vals, x[None], r, p, m)[0]
        got = torch.cat([lm.ell_rows64(tc, tv, tx, a, b, None if r is None else torch.from_numpy(r), p, None if m is None else torch.from_numpy(m))
                         for a, b in lm.spans(M, 16)])
        assert rel_err(got.numpy(), want) < EXACT
    cT, vT = lm.transposed_table(tc, tv)
    K = np.zeros((M, M))
    ok = cols >= 0
    np.add.at(K, (np.repeat(np.arange(M), W).reshape(M, W)[ok], cols[ok]), vals[ok].astype(np.float64))
    KT = np.zeros((M, M))
    np.add.at(KT, (np.repeat(np.arange(M), cT.shape[1]).reshape(M, -1), cT.numpy().astype(np.int64)), vT.numpy().astype(np.float64))
    assert np.array_equal(KT, K.T)
    # the compact copy of a window reproduces the pass at the window's rows
    idx = np.array([0, 3, 17, 40])
    region, local, pos = lm.compact_table(tc, idx, M)
    lv = np.zeros(local.shape, dtype=np.float32)
    lv[pos] = vals[idx]
    small = smoothing_ref.apply_pass(local, lv, x[region][None])[0][pos]
    assert rel_err(small, smoothing_ref.apply_pass(cols, vals, x[None])[0][idx]) < EXACT


def test_attention_references():
    M, W, heads, d = 37, 5, 2, 8
    nbr, _ = _table(M, W, 7)
    for r in range(M):  # the neighbours of a row come first, each once
        u = np.unique(nbr[r][nbr[r] >= 0])
        nbr[r] = -1
        nbr[r, :u.size] = u
    rng = np.random.default_rng(8)
    q, k, v, g = (rng.standard_normal((1, M, d)).astype(np.float32) for _ in range(4))
    rows, cols = np.nonzero(nbr >= 0)[0], nbr[nbr >= 0].astype(np.int64)
    out, dq, dk, dv = attention_ref.attention_grads64(q, k, v, rows, cols, heads, g)
    tq, tk, tv, tg = (torch.from_numpy(a[0]) for a in (q, k, v, g))
    tn = torch.from_numpy(nbr)
    parts = [lm.attention_rows64(tq, tk, tv, tn, a, b, heads, tg) for a, b in lm.spans(M, 10)]
    o64, lse, delta, dq64 = (torch.cat([p[i] for p in parts]) for i in range(4))
    nT = lm.transposed_neighbours(tn)
    dkv = [lm.attention_dkv_rows64(tq, tk, tv, tg, lse, delta, nT, a, b, heads) for a, b in lm.spans(M, 10)]
    dk64, dv64 = (torch.cat([p[i] for p in dkv]) for i in range(2))
    for got, want in ((o64, out[0]), (dq64, dq[0]), (dk64, dk[0]), (dv64, dv[0])):
        assert rel_err(got.numpy(), want) < EXACT
    assert np.all(o64[3].numpy() == 0) and np.all(lse[3].numpy() == 0)  # a row without neighbours


# ---- size limits refused before the first HIP call ------------------------------------------------------------------------------------

def _refused(rc, code, *words):
    msg = _native.last_error()
    assert rc == code and all(w in msg for w in words), (rc, msg)


def test_size_limits_are_refused_before_any_launch():
    """One past each documented limit (include/dsphere.h), at the entry points that check it before they touch the device; the
    pointers are never read.  (dsph_cheb_contract's N <= 65535 is checked behind its device selection and is not probed.)"""
    lib = _native.lib()
    p = 4096  # a non-NULL, 16-byte aligned address
    big = (1 << 40) + 1
    U, B = -3, -1  # DSPH_E_UNSUPPORTED, DSPH_E_BADARG
    _refused(lib.dsph_bn_stats(p, big, 4, 1e-5, p, p, p, None, None, None, None, 0.0, p, 1 << 20, 0, None), U, "bn_stats", "2^40 rows")
    _refused(lib.dsph_bn_stats(p, 1 << 40, 1 << 23, 1e-5, p, p, p, None, None, None, None, 0.0, p, 1 << 20, 0, None), U, "2^62 elements")
    _refused(lib.dsph_bn_apply(p, p, big, 4, p, p, None, None, 0, 0, None), U, "bn_apply", "2^40 rows")
    _refused(lib.dsph_bn_backward(p, None, p, p, p, None, None, None, p, None, None, big, 4, 0, p, 1 << 20, 0, None), U, "bn_backward", "2^40 rows")
    assert lib.dsph_bn_workspace_bytes(big, 4) == 0 and lib.dsph_ln_workspace_bytes(big, 4) == 0
    _refused(lib.dsph_ln_forward(p, None, None, 2 * p, big, 4, 1e-3, None, None, 0, None), U, "ln_forward", "2^40 rows")
    _refused(lib.dsph_ln_backward(p, p, None, None, 1e-3, 2 * p, None, None, big, 4, None, 0, 0, None), U, "ln_backward", "2^40 rows")
    _refused(lib.dsph_patch_gemm(p, p, None, p, big, 4, 4, 4, 0, 0, 0, None), U, "patch_gemm", "2^40 rows")
    _refused(lib.dsph_patch_epilogue_backward(None, p, p, None, big, 4, 4, 0, None, 0, 0, None), U, "patch_epilogue_backward", "2^40 rows")
    assert lib.dsph_patch_backward_workspace_bytes(big, 4, 4) == 0
    _refused(lib.dsph_ell_smooth(p, p, 1 << 31, 9, p, p, 1, 4, None, 0, None, 1, 0, None), B, "ell_smooth", "int32 column indices")
    _refused(lib.dsph_nbr_attention_forward(p, p, p, 64, p, None, p, 9, 1, 1 << 31, 2, 32, 0, None), B, "nbr_attention_forward", "int32 row indices")
    _refused(lib.dsph_nbr_attention_backward(p, p, p, 64, p, p, p, p, 9, p, 9, p, p, p, p, 64, 1, 1 << 31, 2, 32, 0, None), B,
             "nbr_attention_backward", "int32 row indices")
    _refused(lib.dsph_healpix_pool(p, p, 1, 1, 4, (1 << 20) + 1, 0, 0, None), U, "healpix_pool", "too large")
    _refused(lib.dsph_healpix_pool_backward(p, p, p, 1, 1, 4, (1 << 20) + 1, 0, 0, None), U, "healpix_pool", "too large")
