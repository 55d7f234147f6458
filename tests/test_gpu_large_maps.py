"""The map operators past their grid caps (regime A) and past 2^31 elements (regime B), through the C ABI (``pytest -m gpu``).

Every kernel outside the Chebyshev plan -- batch norm, layer norm, the patch GEMM and its epilogue's gradient, pooling, the residual
epilogue, smoothing, neighbour attention, the unfused recurrence step and the row pack / unpack -- at the smallest shape that
crosses each cap of its launcher (the caps and the shapes: DESIGN.md, "Size limits of the map operators"), and at maps of a little
over 2^31 elements, the size a HealpyGCNN at nside 1024 sends through all of them.

The checker is tests/large_map_ref.py (proven on the CPU by tests/test_large_maps_host.py): outputs are NaN-filled views between
sentinel bands, the WHOLE map is swept against plain torch float64 arithmetic on the device, windows of rows (first, last, either
side of the elements at 2^29 / 2^30 / 2^31, both sides of the documented work-split seams, 32 random) go to the host and the numpy
yardsticks of the small-shape tests, inputs are checksummed before and after.  Data is seeded ``torch.randn`` on the device; the rows
a wrapped or dropped region would lose carry +10 in every reduction.  Tolerances are the small-shape tests', unchanged, on the same
measure (``helpers.rel_err``); every figure is printed before it is held to its bound.

Measured on an MI355X (the largest error of each operator over its cases; per case, with time and peak memory: DESIGN.md 4.11):
batch norm 5e-8 statistics, 2e-7 z, 8e-8 gradients; layer norm 2e-7 z, 6e-8 gradients; patch GEMM 1e-6 fp32 and bf16x6, 6e-6 bf16x3,
6e-8 its epilogue's gradient; pooling MAX and both gradients bit for bit, AVG 1e-7; residual epilogue 1e-7; smoothing 5e-7 absolute
against a derived bound of 1.3e-5 or more; neighbour attention 2e-7 forward, 5e-7 gradients; the 64-bit recurrence step 1e-7; pack /
unpack bit for bit.  No test took longer than 2.5 s (``test_headline_config_as_benchmarked``: 2.7 s at its best, 6.4 s as a
process's first test) or more than 76 GB.
"""

import ctypes
import gc
import time

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

pytestmark = pytest.mark.gpu

TOL, TOL_GRAD, TOL_BF16X3, TOL_MOVING, TOL_POOL, TOL_RESIDUAL = 1e-5, 2e-5, 2e-5, 1e-6, 1e-6, 1e-6
BN_EPS, LN_EPS = 1e-5, 1e-3
MEMORY_LIMIT = 96e9
TWO31 = 1 << 31
ROWS_B = (1 << 25) + (1 << 16) + 3  # 33,619,971 rows of 64 channels: 2,151,678,144 elements
CODES = {a: i for i, a in enumerate(lm.ACTS)}
PRECS = {"fp32": _native.PREC_FP32, "bf16x6": _native.PREC_BF16X6, "bf16x3": _native.PREC_BF16X3}


def dev():
    return torch.device("cuda", 0)


def randn(shape, seed):
    return torch.randn(shape, device=dev(), generator=torch.Generator(device=dev()).manual_seed(seed))


def guarded(shape, misalign=0):
    g = lm.Guarded(shape, dev(), misalign)
    return g.view, g.check


def vec(t):
    return torch.as_tensor(np.asarray(t, dtype=np.float32), device=dev())


def held(name, figures, bound):
    """Print every figure, then hold each to its bound."""
    print(f"  {name}: " + ", ".join(f"{k} {v:.2e}" for k, v in figures.items()) + f" (bound {bound:.0e})")
    assert all(v <= bound for v in figures.values()), (name, figures, bound)


@pytest.fixture(autouse=True)
def measured(request):
    """Time and peak device memory of every test, printed; the memory freed afterwards."""
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print(f"[large maps] {request.node.name}: {time.perf_counter() - t0:.1f} s, peak {peak / 1e9:.1f} GB")
    gc.collect()
    torch.cuda.empty_cache()
    assert peak < MEMORY_LIMIT


def vector_width(C, *tensors, allow2=False):
    """The launchers' documented rule (csrc/dsphere_mapops.h: vec_width), restated: the kernels offer no way to observe it."""
    al = 0
    for t in tensors:
        al |= t.data_ptr()
    return 4 if C % 4 == 0 and al % 16 == 0 else 2 if allow2 and C % 2 == 0 and al % 8 == 0 else 1


def ceil_div(a, b):
    return -(-a // b)


# ---- batch norm -------------------------------------------------------------------------------------------------------------------

def bn_backward_into(y, z, dz, stats, gamma, act, dy):
    """``dsph_bn_backward`` with the caller's ``dy`` (``_native.bn_backward`` allocates its own)."""
    rows, F = y.shape
    ws = torch.empty(_native.bn_workspace_bytes(rows, F), dtype=torch.uint8, device=y.device)
    dgamma, dshift = torch.empty(F, device=y.device), torch.empty(F, device=y.device)
    p = _native._ptr
    rc = _native.lib().dsph_bn_backward(p(y), p(z if act != "none" else None), p(dz), p(stats[0]), p(stats[2]), p(stats[3]), p(stats[4]), p(gamma),
                                        p(dy), p(dgamma), p(dshift), rows, F, CODES[act], p(ws), ws.numel(), 0, _native._stream_ptr(y.device))
    _native.check(rc, "dsph_bn_backward")
    return dgamma, dshift


def bn_case(rows, F, acts, bump_from, in_place=False, seed=1):
    """stats (with the moving statistics), apply with every activation of ``acts``, backward with the last of them."""
    step = lm.chunk_rows(F)
    y = randn((rows, F), seed)
    y[bump_from:] += 10.0
    dz = randn((rows, F), seed + 1)
    gamma, shift = 1.0 + 0.2 * randn((F,), seed + 2), 0.3 * randn((F,), seed + 3)
    sums = lm.checksum(y), lm.checksum(dz)
    P = _native.bn_workspace_bytes(rows, F) // (16 * F) - 1
    v = vector_width(F, y, allow2=True)
    rpi = 256 // min(F // v, 256)
    nblk = min(ceil_div(rows, rpi * 16), 16384)
    assert P == 2048 and rows * F > 2048 * 8192, "the partial cap must be crossed"
    assert ceil_div(rows, rpi * 16) > 16384, "the row-block cap of the elementwise kernels must be crossed"
    seams = [rows * b // P for b in (1, 2, P // 2, P - 1)] + [rows * b // nblk for b in (1, nblk // 2 + 1, nblk - 1)]
    idx = lm.window_rows(rows, F, seams=seams, seed=seed)

    rm, rv = torch.zeros(F, device=dev()), torch.ones(F, device=dev())
    stats, _ = _native.bn_stats(y, BN_EPS, rm, rv, momentum=0.1)
    m64, v64 = lm.bn_stats64(y, step)
    mean, var = m64.cpu().numpy(), v64.cpu().numpy()
    want_rm, want_rv = batchnorm_ref.moving_update(np.zeros(F), np.ones(F), mean, var, rows, 0.1)
    rel = lambda got, want: float(np.abs(got.double().cpu().numpy() - want).max() / np.abs(want).max())
    held(f"bn stats ({rows}, {F}) vec {v} P {P}", {"mean": rel(stats[0], mean), "var": rel(stats[1], var),
                                                   "rstd": rel(stats[2], 1 / np.sqrt(var + BN_EPS))}, TOL)
    held("bn moving statistics", {"mean": rel(rm, want_rm), "var": rel(rv, want_rv)}, TOL_MOVING)
    g_np, s_np = gamma.double().cpu().numpy(), shift.double().cpu().numpy()

    z = None
    for act in acts:
        del z
        z, zcheck = guarded((rows, F))
        _native.bn_apply(y, stats[0], stats[2], gamma, shift, act=CODES[act], out=z)
        err, scale = lm.sweep(z, lambda a, b: lm.bn_apply64(y[a:b], m64, v64, BN_EPS, gamma, shift, act), step, f"bn z {act}")
        yard = lambda i: batchnorm_ref._act((lm.host_rows(y, i).astype(np.float64) - mean) / np.sqrt(var + BN_EPS) * g_np + s_np, act)
        held(f"bn apply {act}", {"sweep": err / scale, "windows": lm.windows(z, idx, yard, scale)}, TOL)
        zcheck(f"bn z {act}")
    if in_place:
        yc, ycheck = guarded((rows, F))
        yc.copy_(y)
        assert _native.bn_apply(yc, stats[0], stats[2], gamma, shift, act=CODES[act], out=yc) is yc
        assert lm.equal_sweep(yc, lambda a, b: z[a:b], step, "bn z in place") == 0
        ycheck("bn z in place")
        del yc

    zsum = lm.checksum(z)
    dy, dcheck = guarded((rows, F))
    dgamma, dshift = bn_backward_into(y, z, dz, stats, gamma, act, dy)
    # (relu: the mask of the z under test, as batchnorm_ref.bn_backward does; the smooth activations: the reference's own z)
    z64 = (lambda a, b: lm.f64(z[a:b])) if act == "relu" else (lambda a, b: lm.bn_apply64(y[a:b], m64, v64, BN_EPS, gamma, shift, act))
    s1, s2 = lm.bn_backward_sums64(y, z64, dz, m64, v64, BN_EPS, act, step)
    err, scale = lm.sweep(dy, lambda a, b: lm.bn_dy64(y[a:b], z64(a, b), dz[a:b], m64, v64, BN_EPS, gamma, s1, s2, rows, act), step, "bn dy")
    s1n, s2n = s1.cpu().numpy(), s2.cpu().numpy()

    def yard_dy(i):
        yw, zw = lm.host_rows(y, i).astype(np.float64), lm.host_rows(z, i).astype(np.float64)
        xh = (yw - mean) / np.sqrt(var + BN_EPS)
        zz = zw if act == "relu" else batchnorm_ref._act(xh * g_np + s_np, act)
        g = lm.host_rows(dz, i).astype(np.float64) * batchnorm_ref._act_grad_from_output(zz, act)
        return g_np / np.sqrt(var + BN_EPS) * (g - s1n / rows - xh * s2n / rows)

    held(f"bn backward {act}", {"dy sweep": err / scale, "dy windows": lm.windows(dy, idx, yard_dy, scale), "dgamma": rel(dgamma, s2n),
                                "dshift": rel(dshift, s1n)}, TOL_GRAD)
    dcheck("bn dy")
    assert (lm.checksum(y), lm.checksum(dz)) == sums and lm.checksum(z) == zsum, "an input was written"


def test_bn_past_the_partial_and_row_block_caps_vector():
    """F = 64 (VEC 4, 256 rows per elementwise workgroup): 16,401 row blocks > 16,384 and P = 2048; relu and tanh."""
    rows = (1 << 22) + 4099
    bn_case(rows, 64, ["tanh", "relu"], bump_from=rows * 2047 // 2048)


def test_bn_past_the_partial_and_row_block_caps_scalar():
    """F = 5 (VEC 1, 51 rows per step, 816 per elementwise workgroup): 16,384 * 816 + 4099 rows; sigmoid and elu."""
    rows = 16384 * 816 + 4099
    bn_case(rows, 5, ["sigmoid", "elu"], bump_from=rows * 2047 // 2048, seed=11)


def test_bn_past_2_31_elements():
    rows, F = ROWS_B, 64
    assert rows * F > TWO31
    bn_case(rows, F, ["none"], bump_from=ceil_div(TWO31, F), in_place=True, seed=21)


# ---- layer norm -------------------------------------------------------------------------------------------------------------------

def ln_backward_into(a, dz, dsum, gamma, da):
    rows, d = a.shape
    ws = torch.empty(_native.ln_workspace_bytes(rows, d), dtype=torch.uint8, device=a.device)
    dgamma, dbeta = torch.empty(d, device=a.device), torch.empty(d, device=a.device)
    p = _native._ptr
    rc = _native.lib().dsph_ln_backward(p(a), p(dz), p(dsum), p(gamma), LN_EPS, p(da), p(dgamma), p(dbeta), rows, d, p(ws), ws.numel(), 0,
                                        _native._stream_ptr(a.device))
    _native.check(rc, "dsph_ln_backward")
    return dgamma, dbeta


def ln_case(rows, d, bump_from, seed=31):
    """Forward with residual and affine, backward with dsum and both parameter gradients."""
    step = lm.chunk_rows(d)
    x, res = randn((rows, d), seed), randn((rows, d), seed + 1)
    x[1::3] += 10.0  # rows of mean 10, as layernorm_ref.make_data has them
    gamma, beta = 1.0 + 0.2 * randn((d,), seed + 2), 0.3 * randn((d,), seed + 3)
    sums = lm.checksum(x), lm.checksum(res)
    P = _native.ln_workspace_bytes(rows, d) // (16 * d)
    grid = min(ceil_div(rows * d, 4096), 8192, ceil_div(rows, 4))
    assert P == 2048 and ceil_div(rows * d, 4096) > 8192 and grid == 8192, "the partial cap and the forward's grid cap must be crossed"
    nv = d // 4
    L = min(64, 1 << (nv - 1).bit_length())
    rpb, U = 256 // L, 2 if ceil_div(nv, L) == 1 else 1
    ngroups = ceil_div(rows, rpb)
    seams = []
    for g in (grid, P):  # the first row group of the second and of the last trip of both kernels' grid-stride loops
        assert ngroups > g * U, "a second trip"
        seams += [g * U * rpb, (ngroups - 1) // (g * U) * (g * U) * rpb, g * rpb]
    idx = lm.window_rows(rows, d, seams=seams, seed=seed)

    z, zcheck = guarded((rows, d))
    a, acheck = guarded((rows, d))
    _native.ln_forward(x, gamma, beta, LN_EPS, res=res, out=z, sum_out=a)
    acc_z, acc_a = lm.Accum("ln z"), lm.Accum("ln sum")
    for r0, r1 in lm.spans(rows, step):
        z64, a64 = lm.ln_forward64(x[r0:r1], LN_EPS, gamma, beta, res[r0:r1])
        acc_z.add(z[r0:r1], z64, r0)
        acc_a.add(a[r0:r1], a64, r0)
    g_np, b_np = gamma.cpu().numpy(), beta.cpu().numpy()
    yard = lambda i, k: layernorm_ref.ln_forward(lm.host_rows(x, i), LN_EPS, g_np, b_np, lm.host_rows(res, i))[k]
    held(f"ln forward ({rows}, {d}) grid {grid}", {"z sweep": acc_z.rel, "z windows": lm.windows(z, idx, lambda i: yard(i, 0), acc_z.scale),
                                                   "sum sweep": acc_a.rel, "sum windows": lm.windows(a, idx, lambda i: yard(i, 1), acc_a.scale)}, TOL)
    zcheck("ln z")
    acheck("ln sum")
    assert (lm.checksum(x), lm.checksum(res)) == sums, "an input was written"
    del z, x

    dz, dsum = randn((rows, d), seed + 4), res  # (res serves as the gradient that reached the sum: one map less)
    dz[bump_from:] += 10.0
    sums = lm.checksum(a), lm.checksum(dz), lm.checksum(dsum)
    da, dcheck = guarded((rows, d))
    dgamma, dbeta = ln_backward_into(a, dz, dsum, gamma, da)
    acc = lm.Accum("ln da")
    total = torch.zeros((2, d), dtype=torch.float64, device=dev())
    for r0, r1 in lm.spans(rows, step):
        da64, pg, pb = lm.ln_backward64(a[r0:r1], dz[r0:r1], LN_EPS, gamma, dsum[r0:r1])
        acc.add(da[r0:r1], da64, r0)
        total[0] += pg.sum(dim=0)
        total[1] += pb.sum(dim=0)
    yard_da = lambda i: layernorm_ref.ln_backward(lm.host_rows(a, i), lm.host_rows(dz, i), LN_EPS, g_np, lm.host_rows(dsum, i))[0]
    rel = lambda got, want: float((got.double() - want).abs().max() / want.abs().max())
    held(f"ln backward P {P}", {"da sweep": acc.rel, "da windows": lm.windows(da, idx, yard_da, acc.scale), "dgamma": rel(dgamma, total[0]),
                                "dbeta": rel(dbeta, total[1])}, TOL_GRAD)
    dcheck("ln da")
    assert (lm.checksum(a), lm.checksum(dz), lm.checksum(dsum)) == sums, "an input was written"


def test_ln_past_the_grid_and_partial_caps_d64():
    """d = 64 (16 lanes per row, two row groups in flight): 8,257 > 8,192 workgroups' worth of rows, three trips, P = 2048."""
    rows = (1 << 19) + 4099
    ln_case(rows, 64, bump_from=rows - rows // 5)


def test_ln_past_the_grid_cap_d1024():
    """d = 1024 (a row fills a wave's registers, four vectors per lane): 10,001 row groups on 8,192 workgroups."""
    ln_case(40001, 1024, bump_from=32768, seed=41)


def test_ln_past_2_31_elements():
    assert ROWS_B * 64 > TWO31
    ln_case(ROWS_B, 64, bump_from=ceil_div(TWO31, 64), seed=51)


# ---- the patch GEMM and its epilogue's gradient -------------------------------------------------------------------------------------

def patch_case(R, Kd, C, P, act, resident, precs=("fp32", "bf16x6", "bf16x3"), epilogue=True, seed=61):
    step = lm.chunk_rows(max(Kd, C), lm.CHUNK_ELEMS // 2)
    x = randn((R, Kd), seed)
    w, bias = randn((Kd, C), seed + 1) / float(np.sqrt(Kd)), randn((P,), seed + 2)
    sums = lm.checksum(x), lm.checksum(w)
    ngroups = ceil_div(R, 256)
    lds = {p: ceil_div(Kd, 16) * ceil_div(C, 32) * (3072 if p == "bf16x6" else 2048) for p in precs}  # (csrc/patch_gemm.hip: a.resident)
    assert ngroups > 1024, "a second trip of the persistent loop"
    assert all((lds[p] <= 96 * 1024) == resident for p in precs), lds
    idx = lm.window_rows(R, max(Kd, C), seams=[1024 * 256, (ngroups - 1) // 1024 * 1024 * 256], seed=seed)
    outs = {}
    for p in precs:
        outs[p] = guarded((R, C))
        _native.patch_gemm(x, w, bias, P, act=CODES[act], precision=PRECS[p], out=outs[p][0])
    accs = {p: lm.Accum(f"patch y {p}") for p in precs}
    for r0, r1 in lm.spans(R, step):  # the reference once per chunk, shared by the three arithmetics
        y64 = lm.patch_forward64(x[r0:r1], w, bias, P, act)
        for p in precs:
            accs[p].add(outs[p][0][r0:r1], y64, r0)
    w_np, b_np = w.cpu().numpy(), bias.cpu().numpy()
    yard = lambda i: pseudoconv_ref.patch_forward(lm.host_rows(x, i), w_np, b_np, P, act)
    for p in precs:
        held(f"patch gemm ({R}, {Kd}, {C}, {P}) {act} {p} {'resident' if resident else 're-staged'}",
             {"sweep": accs[p].rel, "windows": lm.windows(outs[p][0], idx, yard, accs[p].scale)}, TOL_BF16X3 if p == "bf16x3" else TOL)
        outs[p][1](f"patch y {p}")
    assert (lm.checksum(x), lm.checksum(w)) == sums, "an input was written"
    if not epilogue:
        return
    y = outs[precs[0]][0]
    del x
    dy = randn((R, C), seed + 3)
    dy[R - R // 5:] += 10.0
    NP = _native.patch_backward_workspace_bytes(R, C, P) // (8 * P)
    assert NP == 2048 and R * C > 2048 * 8192, "the epilogue's partial cap must be crossed"
    sums = lm.checksum(y), lm.checksum(dy)
    dz, dcheck = guarded((R, C))
    _, dbias, _ = _native.patch_epilogue_backward(y, dy, P, act=CODES[act], out=dz)
    stepc = lm.chunk_rows(C)
    err, scale = lm.sweep(dz, lambda a, b: lm.patch_dz64(y[a:b], dy[a:b], act), stepc, "patch dz")
    db64 = lm.chunked_sum(lambda a, b: lm.patch_dz64(y[a:b], dy[a:b], act).reshape(b - a, C // P, P).sum(dim=1), R, stepc)
    yard_dz = lambda i: lm.host_rows(dy, i).astype(np.float64) * pseudoconv_ref._act_grad_from_output(lm.host_rows(y, i).astype(np.float64), act)
    held(f"patch epilogue backward NP {NP}", {"dz sweep": err / max(scale, 1e-300), "dz windows": lm.windows(dz, idx, yard_dz, scale),
                                              "dbias": float((dbias.double() - db64).abs().max() / db64.abs().max())}, TOL_GRAD)
    dcheck("patch dz")
    assert (lm.checksum(y), lm.checksum(dy)) == sums, "an input was written"


R_A = (1 << 18) + 513  # 262,657 rows: 1,027 groups of 256 on 1,024 workgroups, and R * 64 > 2048 * 8192


def test_patch_gemm_second_trip_resident():
    patch_case(R_A, 256, 64, 64, "relu", resident=True)


def test_patch_gemm_second_trip_restaged():
    """W does not fit the LDS: every trip of the persistent loop re-enters the barrier pair of the staging (C = 32: the epilogue's
    partial cap is not reached at this R; the other two cases cross it)."""
    patch_case(R_A, 1024, 32, 32, "none", resident=False, epilogue=False, seed=71)


def test_patch_gemm_second_trip_transpose_periodic_bias():
    patch_case(300001, 64, 256, 64, "elu", resident=True, seed=81)


def test_patch_gemm_x_past_2_31_elements():
    R = (1 << 23) + (1 << 14) + 3
    assert R * 256 > TWO31
    patch_case(R, 256, 64, 64, "relu", resident=True, seed=91)


def test_patch_gemm_y_past_2_31_elements():
    R = (1 << 23) + (1 << 14) + 3
    assert R * 256 > TWO31
    patch_case(R, 64, 256, 64, "relu", resident=True, seed=101)


# ---- pooling ------------------------------------------------------------------------------------------------------------------------

def pool_into(x, y, rows_out, F, group, kind):
    rc = _native.lib().dsph_healpix_pool(_native._ptr(x), _native._ptr(y), 1, rows_out, F, group, _native.POOL_MAX if kind == "MAX" else _native.POOL_AVG,
                                         0, _native._stream_ptr(x.device))
    _native.check(rc, "dsph_healpix_pool")


def pool_backward_into(x, dy, dx, rows_out, F, group, kind):
    rc = _native.lib().dsph_healpix_pool_backward(_native._ptr(x), _native._ptr(dy), _native._ptr(dx), 1, rows_out, F, group,
                                                  _native.POOL_MAX if kind == "MAX" else _native.POOL_AVG, 0, _native._stream_ptr(x.device))
    _native.check(rc, "dsph_healpix_pool_backward")


def pool_case(rows_out, F, group, kinds, seed=111):
    """Seeded normal data: a tie inside a group is possible at this size, and the reference sends the gradient to the FIRST child
    that holds the maximum, as the kernel documents, so ties are part of the check, not a hazard."""
    step = lm.chunk_rows(F * group)
    x = randn((rows_out * group, F), seed)
    dy = randn((rows_out, F), seed + 1)
    sums = lm.checksum(x), lm.checksum(dy)
    v = vector_width(F, x)
    assert rows_out * (F // v) > 1 << 28 and rows_out * F > 1 << 28, "a second trip of both grid-stride loops (2^20 workgroups of 256)"
    idx = lm.window_rows(rows_out, F * group, seams=[(1 << 28) // (F // v), (1 << 28) // F], seed=seed)
    x_of = lambda i: lm.host_rows(x.view(rows_out, group, F), i).astype(np.float64)
    for kind in kinds:
        y, ycheck = guarded((rows_out, F))
        pool_into(x, y, rows_out, F, group, kind)
        if kind == "MAX":
            wrong = lm.equal_sweep(y, lambda a, b: lm.pool_forward64(x[a * group:b * group], group, "MAX"), step, "pool y")
            win = lm.windows(y, idx, lambda i: x_of(i).max(axis=1))
            print(f"  pool MAX ({rows_out}, {F}) group {group} vec {v}: {wrong} elements differ, windows {win:.2e}")
            assert wrong == 0 and win == 0
        else:
            err, scale = lm.sweep(y, lambda a, b: lm.pool_forward64(x[a * group:b * group], group, "AVG"), step, "pool y")
            held(f"pool AVG ({rows_out}, {F}) group {group} vec {v}", {"sweep": err / scale, "windows": lm.windows(y, idx, lambda i: x_of(i).mean(axis=1), scale)},
                 TOL_POOL)
        ycheck("pool y")
        del y
        dx, dcheck = guarded((rows_out * group, F))
        pool_backward_into(x, dy, dx, rows_out, F, group, kind)
        wrong = lm.equal_sweep(dx.view(rows_out, group * F),
                               lambda a, b: lm.pool_backward32(x[a * group:b * group], dy[a:b], group, kind).reshape(b - a, group * F), step, "pool dx")
        print(f"  pool {kind} backward: {wrong} elements differ")
        assert wrong == 0
        dcheck("pool dx")
        del dx
    assert (lm.checksum(x), lm.checksum(dy)) == sums, "an input was written"


def test_pool_second_trip_scalar():
    pool_case(89480001, 3, 4, ["MAX", "AVG"])


def test_pool_second_trip_scalar_p2():
    pool_case(89480001, 3, 16, ["MAX"], seed=121)


@pytest.mark.parametrize("kind", ["MAX", "AVG"])
def test_pool_second_trip_vector_and_x_past_2_32_elements(kind):
    """F = 64, group 4: rows_out * 16 > 2^28 makes x 4.3e9 elements -- regime A of the vector kernel is regime B of its input."""
    rows_out = (1 << 24) + 4099
    assert rows_out * 4 * 64 > 2 * TWO31
    pool_case(rows_out, 64, 4, [kind], seed=131)


# ---- the residual epilogue --------------------------------------------------------------------------------------------------------------

def residual_case(n, misalign, act, before, seed=141):
    step = lm.CHUNK_ELEMS
    y, ycheck = guarded((n,), misalign)
    y.copy_(randn((n,), seed))
    skip = randn((n,), seed + 1)
    ssum = lm.checksum(skip)
    vec4 = misalign == 0
    work = ceil_div(n, 4) if vec4 else n
    assert ceil_div(work, 256) > 8192, "second trips on the 8,192 workgroups"
    assert not vec4 or n % 4 != 0, "a scalar tail behind the float4 body"
    stride = 8192 * 256
    idx = lm.window_rows(n, 1, seams=[stride * (4 if vec4 else 1), n // 4 * 4, (work - 1) // stride * stride * (4 if vec4 else 1)], seed=seed)
    assert _native.residual_epilogue(y, skip, 0.25, CODES[act], before) is y
    y0 = randn((n,), seed)  # the input again, from its seed
    err, scale = lm.sweep(y, lambda a, b: lm.residual64(y0[a:b], skip[a:b], 0.25, act, before), step, "residual y")

    def yard(i):
        a, b = lm.host_rows(y0, i).astype(np.float64), lm.host_rows(skip, i).astype(np.float64)
        return batchnorm_ref._act(a, act) + 0.25 * b if before else batchnorm_ref._act(a + 0.25 * b, act)

    held(f"residual epilogue n {n} misalign {misalign} {act} before {before}", {"sweep": err / scale, "windows": lm.windows(y, idx, yard, scale)}, TOL_RESIDUAL)
    ycheck("residual y")
    assert lm.checksum(skip) == ssum, "skip was written"


@pytest.mark.parametrize("misalign,act,before", [(0, "relu", False), (0, "tanh", True), (1, "tanh", False), (1, "relu", True)])
def test_residual_epilogue_second_trips_and_tail(misalign, act, before):
    residual_case((1 << 23) + (1 << 21) + 3, misalign, act, before)


def test_residual_epilogue_past_2_31_elements():
    n = ROWS_B * 64 + 3
    assert n > TWO31
    residual_case(n, 0, "relu", False, seed=151)


# ---- the unfused recurrence step: cheb_step_kernel<1, uint64_t> -------------------------------------------------------------------------

def test_cheb_step_64_bit_index_instantiation():
    """The nside-1024 grid plan, F = 173, N = 1: rows * F = 2,176,843,776 >= 2^31 - 256 and F odd, so ``launch_cheb_step`` takes
    ``cheb_step_kernel<1, uint64_t>`` (csrc/cheb_step.hip; the tiled step serves only the wide graphs and is switched off here
    besides).  alpha = 2, beta = 1 with ``prev``: one step of the Chebyshev recurrence."""
    import bench
    from test_gpu_round2 import _patch_reference

    cols, vals, _ = bench.build_laplacian(1024, dev())
    M, F = cols.shape[0], 173
    assert M * F > TWO31 and F % 4 != 0
    plan = _native.LaplacianPlan(cols, vals, device=0, options={_native.OPT_TSTEP: 0})
    inp, prev = randn((1, M, F), 161), randn((1, M, F), 162)
    sums = lm.checksum(inp), lm.checksum(prev)
    out, check = guarded((1, M, F))
    assert _native.cheb_step(plan, inp, prev, 2.0, 1.0, out=out) is out
    dc, dv = torch.as_tensor(cols, device=dev()), torch.as_tensor(vals, device=dev())
    err, scale = lm.sweep(out[0], lambda a, b: 2.0 * lm.ell_rows64(dc, dv, inp[0], a, b) - lm.f64(prev[0, a:b]), lm.chunk_rows(9 * F), "cheb step")
    idx = lm.window_rows(M, F, seed=161)
    W1 = np.zeros((2 * F, F))
    W1[2 * np.arange(F) + 1, np.arange(F)] = 1.0  # y = T_1 x = L~ x out of the two-term oracle

    def yard(i):
        return 2.0 * _patch_reference(cols, vals, inp, W1, 2, i)[0] - lm.host_rows(prev[0], i).astype(np.float64)

    held(f"cheb step ({M}, {F}) uint64", {"sweep": err / scale, "windows": lm.windows(out[0], idx, yard, scale)}, TOL)
    check("cheb step out")
    assert (lm.checksum(inp), lm.checksum(prev)) == sums, "an input was written"


# ---- row pack / unpack --------------------------------------------------------------------------------------------------------------------

def test_rows_pack_unpack_past_2_31_elements():
    N, rows, F = 2, (1 << 24) + 77, 65
    assert N * rows * F > TWO31 and (N - 1) * rows * F < TWO31 < ((N - 1) * rows + rows - 1) * F
    src = randn((N, rows, F), 171)
    ssum = lm.checksum(src)
    rng = np.random.default_rng(171)
    pick = np.unique(np.concatenate([[0, 1, rows - 1, rows - 2, (TWO31 // F) % rows, (TWO31 // F) % rows + 1], rng.integers(0, rows, size=100003)]))
    idx = torch.as_tensor(rng.permutation(pick).astype(np.int32), device=dev())
    buf, bcheck = guarded((N, idx.numel(), F))
    assert _native.rows_pack(src, idx, out=buf) is buf
    want = src[:, idx.long()]
    assert bool(torch.isfinite(buf).all()) and torch.equal(buf.view(torch.int32), want.view(torch.int32)), "pack is not bit for bit"
    bcheck("packed rows")
    dst, dcheck = guarded((N, rows, F))
    dst.fill_(1.5)
    _native.rows_unpack(dst, idx, buf)
    assert torch.equal(dst[:, idx.long()].view(torch.int32), want.view(torch.int32)), "the round trip is not bit for bit"
    touched = sum(int((dst[n] != 1.5).sum()) for n in range(N))
    assert touched == int((want != 1.5).sum()), "unpack wrote rows it was not given"
    dcheck("unpacked rows")
    assert lm.checksum(src) == ssum, "src was written"
    print(f"  rows pack / unpack ({N}, {rows}, {F}), {idx.numel()} rows: bit for bit")


# ---- smoothing ----------------------------------------------------------------------------------------------------------------------------

M_B = (1 << 22) + 77  # 4,194,381 rows


def local_table(M, W, seed, neighbours_first=False):
    """A synthetic table on the device, as tests/test_gpu_smoothing.py builds its own: columns within 2,048 rows of the row (as a
    smoothing kernel's are), about a tenth of the slots empty (-1; their weights stay and must not count), weights nonnegative and
    every row summing to 1 over its valid entries.  ``neighbours_first``: a neighbour table -- the empty slots at the end of the row."""
    gen = torch.Generator(device=dev()).manual_seed(seed)
    off = torch.randint(-2048, 2049, (M, W), generator=gen, device=dev(), dtype=torch.int32)
    cols = torch.remainder(torch.arange(M, device=dev(), dtype=torch.int32).unsqueeze(1) + off, M)
    del off
    if neighbours_first:
        count = torch.randint(0, W + 1, (M, 1), generator=gen, device=dev(), dtype=torch.int32)
        empty = torch.arange(W, device=dev(), dtype=torch.int32).unsqueeze(0) >= count
    else:
        empty = torch.rand((M, W), generator=gen, device=dev()) < 0.1
    cols[empty] = -1
    vals = torch.rand((M, W), generator=gen, device=dev()) + 1e-3
    norm = torch.where(empty, torch.zeros((), device=dev()), vals).sum(dim=1, keepdim=True)
    vals = vals / torch.where(norm > 0, norm, torch.ones((), device=dev()))
    return cols, vals


def smooth_bound(W, scale):
    return 2 * (W + 8) * 2.0 ** -24 * scale  # tests/test_gpu_smoothing.py: bound(W, 1, scale)


def smooth_check(cols, vals, x, reps, mask, name, scale_factor=1.0, seed=0, maps=None):
    """One pass over all N maps; ``maps``: the maps this test sweeps (None: all) -- the float64 sweep of a 130-wide table over 2.4e9
    elements takes longer than a test may, so the tests of that table share it out, each running the whole pass."""
    N, M, C = x.shape
    W = cols.shape[1]
    maps = range(N) if maps is None else maps
    xsum = lm.checksum(x)
    y, ycheck = guarded((N, M, C))
    assert _native.ell_smooth(cols, vals, x, out=y, reps=reps, pass_index=0, mask=mask) is y
    acc = lm.Accum(name)
    for n in maps:
        for r0, r1 in lm.spans(M, lm.chunk_rows(W * C)):
            acc.add(y[n, r0:r1], lm.ell_rows64(cols, vals, x[n], r0, r1, reps, 0, mask), n * M + r0)
    assert all(bool(torch.isfinite(y[n]).all()) for n in range(N)), "a NaN pre-fill or another non-finite number is left in y"
    tol = smooth_bound(W, float(x.abs().max()) * scale_factor)
    win = 0.0
    rows = lm.window_rows(N * M, C, seed=seed)
    reps_np = None if reps is None else reps.cpu().numpy()
    for n in np.intersect1d(np.unique(rows // M), np.asarray(list(maps))):
        idx = rows[rows // M == n] % M
        region, local, pos = lm.compact_table(cols, idx, M)
        lv = np.zeros(local.shape, dtype=np.float32)
        lv[pos] = lm.host_rows(vals, idx)
        mk = None if mask is None else lm.host_rows(mask, region)
        want = smoothing_ref.apply_pass(local, lv, lm.host_rows(x[n], region)[None], reps_np, 0, mk)[0][pos]
        win = max(win, float(np.abs(lm.host_rows(y[n], idx).astype(np.float64) - want).max()))
    print(f"  {name} M {M} W {W} C {C} N {N}: sweep err {acc.err:.3e}, windows {win:.3e}, bound {tol:.3e}")
    assert acc.err <= tol and win <= tol
    ycheck(name)
    assert lm.checksum(x) == xsum, "x was written"


@pytest.mark.parametrize("W,maps", [(9, None), (-9, None), (130, (0, 1)), (130, (2, 3)), (130, (4, 5)), (130, (6, 7)), (130, (8,))],
                         ids=["w9", "w9-transposed", "w130-maps01", "w130-maps23", "w130-maps45", "w130-maps67", "w130-map8"])
def test_smoothing_last_map_past_2_31_elements(W, maps):
    """W = 9: 16 lanes per row, with ``reps`` (a quarter of the channels passed through) and an [M, 1] mask; its transposed table
    (the input gradient's pass); W = 130: 64 lanes per row, three entries per lane, the sweep of its nine maps shared out."""
    N, M, C = 9, M_B, 64
    assert (N - 1) * M * C > TWO31, "the last map starts past 2^31 elements"
    cols, vals = local_table(M, abs(W), 181 + abs(W))
    x = randn((N, M, C), 191 + abs(W))
    if W == 130:
        smooth_check(cols, vals, x, None, None, "smooth 64 lanes", seed=W, maps=maps)
    elif W == 9:
        reps = torch.as_tensor(np.where(np.arange(C) % 4 == 1, 0, 1).astype(np.int32), device=dev())
        mask = torch.rand((M, 1), device=dev(), generator=torch.Generator(device=dev()).manual_seed(5))
        smooth_check(cols, vals, x, reps, mask, "smooth 16 lanes, reps, mask", seed=W)
    else:
        colsT, valsT = lm.transposed_table(cols, vals)
        del cols, vals
        S = float(valsT.sum(dim=1).max())
        assert abs(W) <= colsT.shape[1] <= 128, "the transposed table stays in the 16-lane class"
        smooth_check(colsT, valsT, x, None, None, f"smooth transposed (S {S:.2f})", scale_factor=max(S, 1.0), seed=10)


# ---- neighbour attention ------------------------------------------------------------------------------------------------------------------

HEADS, DEPTH = 2, 32


def attention_forward_into(q, k, v, nbr, out, lse):
    ld, N, M, d = _native._qkv_layout(q, k, v, HEADS)
    p = _native._ptr
    rc = _native.lib().dsph_nbr_attention_forward(p(q), p(k), p(v), ld, p(out), p(lse), p(nbr), int(nbr.shape[1]), N, M, HEADS, DEPTH, 0,
                                                  _native._stream_ptr(q.device))
    _native.check(rc, "dsph_nbr_attention_forward")
    return ld


def attention_windows(q, k, v, nbr, out, dout, dq, seed, maps=None):
    """out (and dq) at the window rows (of ``maps``; None: of every map) against ``attention_ref`` on a compact copy of the rows and
    their neighbours: -> the largest absolute errors.  (dk and dv of a row need its in-edges' whole rows, two hops out: the sweep
    alone holds them.)"""
    N, M, d = out.shape
    rows = lm.window_rows(N * M, d, seed=seed)
    eo = eq = 0.0
    for n in np.intersect1d(np.unique(rows // M), np.arange(N) if maps is None else np.asarray(maps)):
        idx = rows[rows // M == n] % M
        region, local, pos = lm.compact_table(nbr, idx, M)
        er, ec = np.nonzero(local >= 0)[0], local[local >= 0]
        qs, ks, vs = (lm.host_rows(t[n], region)[None] for t in (q, k, v))
        if dout is None:
            want = attention_ref.attention_np(qs, ks, vs, er, ec, HEADS)[0][0][pos]
        else:
            g = np.zeros(qs.shape, dtype=np.float32)
            g[0, pos] = lm.host_rows(dout[n], idx)
            o, gq, _, _ = attention_ref.attention_grads64(qs, ks, vs, er, ec, HEADS, g)
            want = o[0][pos]
            eq = max(eq, float(np.abs(lm.host_rows(dq[n], idx).astype(np.float64) - gq[0][pos]).max()))
        eo = max(eo, float(np.abs(lm.host_rows(out[n], idx).astype(np.float64) - want).max()))
    return eo, eq


def test_nbr_attention_forward_contiguous_past_2_31_elements():
    N, M, d = 8, M_B, HEADS * DEPTH
    assert N * M * d > TWO31
    nbr, _ = local_table(M, 9, 201, neighbours_first=True)
    q, k, v = (randn((N, M, d), 211 + i) for i in range(3))
    sums = [lm.checksum(t) for t in (q, k, v)]
    out, ocheck = guarded((N, M, d))
    lse, lcheck = guarded((N, M, HEADS))
    assert attention_forward_into(q, k, v, nbr, out, lse) == d
    ao, al = lm.Accum("attention out"), lm.Accum("attention lse")
    for n in range(N):
        for r0, r1 in lm.spans(M, lm.chunk_rows(9 * d * 2)):
            o64, l64 = lm.attention_rows64(q[n], k[n], v[n], nbr, r0, r1, HEADS)
            ao.add(out[n, r0:r1], o64, n * M + r0)
            al.add(lse[n, r0:r1], l64, n * M + r0)
    eo, _ = attention_windows(q, k, v, nbr, out, None, None, 211)
    held(f"nbr attention forward ({N}, {M}, {d}) contiguous", {"out sweep": ao.rel, "out windows": eo / ao.scale, "lse sweep": al.rel}, TOL)
    ocheck("attention out")
    lcheck("attention lse")
    assert [lm.checksum(t) for t in (q, k, v)] == sums, "an input was written"


class TestNbrAttentionPackedPast2_31Elements:
    """q | k | v as three views of one (N, M, 3 d) projection (row stride 3 d), the gradients into three views of one buffer: the
    layout the layer uses, and the one that keeps the eight map tensors of the backward inside the memory limit.  Forward and
    backward run ONCE on all eight maps (the class's fixture: 69 GB of map tensors are allocated once, and nothing writes them
    afterwards); the float64 sweep of all eight maps takes longer than a test may, so four tests share it, two maps each."""

    N, M, d = 8, M_B, HEADS * DEPTH

    @pytest.fixture(scope="class")
    def run(self):
        N, M, d = self.N, self.M, self.d
        nbr, _ = local_table(M, 9, 221, neighbours_first=True)
        nbrT = lm.transposed_neighbours(nbr)
        qkv = randn((N, M, 3 * d), 231)
        q, k, v = (qkv[..., i * d:(i + 1) * d] for i in range(3))
        dout = randn((N, M, d), 232)
        sums = lm.checksum(qkv), lm.checksum(dout)
        out, ocheck = guarded((N, M, d))
        lse, lcheck = guarded((N, M, HEADS))
        ld = attention_forward_into(q, k, v, nbr, out, lse)
        grads, gcheck = guarded((N, M, 3 * d))
        dq, dk, dv = (grads[..., i * d:(i + 1) * d] for i in range(3))
        _native.nbr_attention_backward(q, k, v, out, lse, dout, nbr, nbrT, HEADS, grads=(dq, dk, dv))
        torch.cuda.synchronize()
        state = dict(nbr=nbr, nbrT=nbrT, qkv=qkv, q=q, k=k, v=v, dout=dout, sums=sums, out=out, lse=lse, grads=grads, dq=dq, dk=dk, dv=dv,
                     ld=ld, checks=((ocheck, "attention out"), (lcheck, "attention lse"), (gcheck, "attention gradients")))
        del nbr, nbrT, qkv, q, k, v, dout, out, lse, grads, dq, dk, dv
        yield state
        state.clear()
        gc.collect()
        torch.cuda.empty_cache()

    def test_outputs_written_bands_and_inputs_untouched(self, run):
        N, M, d = self.N, self.M, self.d
        assert N * M * d > TWO31 and run["ld"] == 3 * d and run["q"].stride(1) == 3 * d
        assert all(bool(torch.isfinite(run[t][n]).all()) for t in ("out", "lse", "grads") for n in range(N)), "a NaN pre-fill is left in an output"
        for check, what in run["checks"]:
            check(what)
        assert (lm.checksum(run["qkv"]), lm.checksum(run["dout"])) == run["sums"], "an input was written"

    @pytest.mark.parametrize("maps", [(0, 1), (2, 3), (4, 5), (6, 7)], ids=["maps01", "maps23", "maps45", "maps67"])
    def test_sweep(self, run, maps):
        N, M, d = self.N, self.M, self.d
        q, k, v, dout, nbr, nbrT = (run[t] for t in ("q", "k", "v", "dout", "nbr", "nbrT"))
        out, lse, dq, dk, dv = (run[t] for t in ("out", "lse", "dq", "dk", "dv"))
        acc = {name: lm.Accum(f"attention {name}") for name in ("out", "lse", "dq", "dk", "dv")}
        WT = nbrT.shape[1]
        for n in maps:
            lse64 = torch.empty((M, HEADS), dtype=torch.float64, device=dev())
            delta64 = torch.empty((M, HEADS), dtype=torch.float64, device=dev())
            for r0, r1 in lm.spans(M, lm.chunk_rows(9 * d * 2)):
                o64, l64, d64, dq64 = lm.attention_rows64(q[n], k[n], v[n], nbr, r0, r1, HEADS, dout[n])
                lse64[r0:r1], delta64[r0:r1] = l64, d64
                acc["out"].add(out[n, r0:r1], o64, n * M + r0)
                acc["lse"].add(lse[n, r0:r1], l64, n * M + r0)
                acc["dq"].add(dq[n, r0:r1], dq64, n * M + r0)
            for r0, r1 in lm.spans(M, lm.chunk_rows(WT * d * 2)):
                dk64, dv64 = lm.attention_dkv_rows64(q[n], k[n], v[n], dout[n], lse64, delta64, nbrT, r0, r1, HEADS)
                acc["dk"].add(dk[n, r0:r1], dk64, n * M + r0)
                acc["dv"].add(dv[n, r0:r1], dv64, n * M + r0)
        eo, eq = attention_windows(q, k, v, nbr, out, dout, dq, 231, maps)
        held(f"nbr attention forward ({N}, {M}, {d}) packed, maps {maps}", {"out sweep": acc["out"].rel, "out windows": eo / acc["out"].scale,
                                                                           "lse sweep": acc["lse"].rel}, TOL)
        held(f"nbr attention backward, transposed width {WT}", {"dq sweep": acc["dq"].rel, "dq windows": eq / acc["dq"].scale,
                                                                "dk sweep": acc["dk"].rel, "dv sweep": acc["dv"].rel}, TOL_GRAD)
        assert (lm.checksum(run["qkv"]), lm.checksum(dout)) == run["sums"], "an input was written"

