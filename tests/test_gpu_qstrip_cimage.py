"""The K = 5 quad strips' packed image of L~ (DSPH_OPT_QSTRIP_IMAGE; csrc/cheb_qstrip.hip, qstrip_cimage_kernel): the ring rows
of every strip, built once per plan and basis and moved into the kernel's LDS ring by LDS-DMA instead of being gathered, doubled
and filed by the H waves in every step.  The ring holds the same floats either way and no arithmetic changes its order, so y with
the image is BITWISE equal to y without it; every case checks that, and the whole map against the float64 oracle at the project's
1e-5.  Quad strips are forced on (DSPH_OPT_STRIPS = always): these maps are too small for the cost rule."""

import numpy as np
import pytest
import torch

from deepsphere import _native
from helpers import rel_err
from oracle import cheb_oracle as orc
from test_gpu_round3 import _csr, _dev, _grid_ell

pytestmark = pytest.mark.gpu
TOL = 1e-5
K, FIN = 5, 64
IMG_ON, IMG_OFF = 1, 2
_DX = (-1, -1, 0, 1, 1, 1, 0, -1)  # W NW N NE E SE S SW (kDirX / kDirY)
_DY = (0, 1, 1, 1, 0, -1, -1, -1)


def _plan(cols, vals, Fout=64):
    plan = _native.LaplacianPlan(cols, vals, device=0, options={_native.OPT_STRIPS: _native.STRIPS_ALWAYS,
                                                                 _native.OPT_QSTRIP_IMAGE: IMG_ON})
    plan.prepare(K, FIN, Fout=Fout)
    return plan


def _inputs(M, N, Fout, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, M, FIN)).astype(np.float32)
    W = (rng.standard_normal((FIN * K, Fout)) * orc.default_kernel_stddev(FIN, K)).astype(np.float32)
    b = rng.standard_normal(Fout).astype(np.float32)
    return x, W, b


def _on_off_oracle(cols, vals, N, Fout, seed, basis="chebyshev", act=None, bias=False, precision=None, what=""):
    """image on == image off bit for bit, and the whole map against the oracle"""
    precision = _native.PREC_BF16X3 if precision is None else precision
    M = cols.shape[0]
    x, W, b = _inputs(M, N, Fout, seed)
    fwd = orc.chebyshev_forward if basis == "chebyshev" else orc.monomial_forward
    ref = fwd(_csr(cols, vals), x, W, K, bias=b if bias else None, activation=act)
    plan = _plan(cols, vals, Fout)
    assert plan.strip_tiles(FIN, Fout, K, precision, N=N) > 0, "no tile on the quad strips"
    B = {"chebyshev": _native.BASIS_CHEBYSHEV, "monomial": _native.BASIS_MONOMIAL}[basis]
    kw = dict(act=_native.ACT_RELU if act == "relu" else _native.ACT_NONE, precision=precision, algo=_native.ALGO_FUSED, basis=B)
    xd, Wd, bd = _dev(x), _dev(W), (_dev(b) if bias else None)
    y_on, _ = _native.cheb_forward(plan, xd, Wd, bd, K, **kw)
    assert plan.strip_image(0, basis=B).size > 0  # (the image of this basis exists: the forward above ran on it)
    plan.set_option(_native.OPT_QSTRIP_IMAGE, IMG_OFF)
    y_off, _ = _native.cheb_forward(plan, xd, Wd, bd, K, **kw)
    err = rel_err(y_on.cpu().numpy(), ref)
    print(f"{what}: M {M}, N {N}, {FIN} -> {Fout}, {basis}: image on vs off equal {torch.equal(y_on, y_off)}, rel err {err:.2e}")
    assert torch.equal(y_on, y_off), "the image path must leave the bits of the gather path"
    assert err < TOL
    return plan


@pytest.fixture(scope="module")
def grid64():
    return _grid_ell(64)


def test_full_sphere_odd_batch(grid64):
    """nside 64: the smallest map whose strips cross equatorial-polar base-pixel borders through the tables and whose tape is cut
    mid-strip; batch 3: the workgroups do not divide evenly into maps."""
    _on_off_oracle(*grid64, N=3, Fout=64, seed=643, what="nside 64")


def test_two_column_blocks_bias_relu(grid64):
    _on_off_oracle(*grid64, N=1, Fout=128, seed=641, act="relu", bias=True, what="nside 64, two column blocks")


def test_monomial_basis(grid64):
    """the image as it stands (not doubled), and the kernel variant whose H waves file x alone"""
    _on_off_oracle(*grid64, N=2, Fout=64, seed=642, basis="monomial", what="nside 64")


def test_f16_three_term_split(grid64):
    _on_off_oracle(*grid64, N=2, Fout=64, seed=644, precision=_native.PREC_F16X3, act="relu", bias=True, what="nside 64 f16x3")


@pytest.mark.parametrize("drop", [100, 200, 256 + 37])
def test_truncated_sphere_with_an_incomplete_last_tile(drop):
    """A sphere cut off `drop` pixels before its end (the map of test_quad_strips_on_a_map_with_an_incomplete_last_tile): the image
    holds rows past the strips' halo (ylo - 1, yhi + 1 .. yhi + 6), which must exist in the map."""
    cols, vals = _grid_ell(128)
    M = cols.shape[0] - drop
    cols, vals = cols[:M].copy(), vals[:M].copy()
    gone = cols >= M
    vals[gone] = 0.0
    cols[gone] = np.broadcast_to(np.arange(M, dtype=cols.dtype)[:, None], cols.shape)[gone]
    plan = _on_off_oracle(cols, vals, N=2, Fout=64, seed=drop, act="relu", bias=True, what=f"nside 128 without its last {drop} pixels")
    rec = plan.strip_pairs(K)
    plan.set_option(_native.OPT_QSTRIP_IMAGE, IMG_ON)
    for s in (0, rec.shape[0] - 1):
        img = plan.strip_image(s)
        assert img.shape[0] == int(rec[s, 11]) - int(rec[s, 10]) + 8 and np.isfinite(img).all()


def test_partial_sky_cap():
    """The cap of 1/3 of the sphere at nside 128 padded to nside-8 superpixels (the construction of bench.py --config c5 at a small
    size): many short strips, many run-ins."""
    import bench

    cols, vals, _ = bench.build_laplacian_masked(128, torch.device("cuda", 0), nside_super=8)
    _on_off_oracle(cols, vals, N=2, Fout=64, seed=1288, what="nside 128 cap")


def test_option_flip_and_graph_replay(grid64):
    """Two forwards on one plan with the option flipped in between (the image freed and rebuilt), then a torch.cuda.graph replay of
    the image path: the image exists before the capture, the replay equals the eager forward."""
    cols, vals = grid64
    M, N, Fout = cols.shape[0], 2, 64
    x, W, b = _inputs(M, N, Fout, 645)
    xd, Wd, bd = _dev(x), _dev(W), _dev(b)
    plan = _plan(cols, vals)
    kw = dict(act=_native.ACT_RELU, precision=_native.PREC_BF16X3, algo=_native.ALGO_FUSED)
    y_on, ws = _native.cheb_forward(plan, xd, Wd, bd, K, **kw)
    kw["workspace"] = ws  # (the capture below allocates nothing)
    plan.set_option(_native.OPT_QSTRIP_IMAGE, IMG_OFF)
    with pytest.raises(RuntimeError):
        plan.strip_image(0)  # (off: no image)
    y_off, _ = _native.cheb_forward(plan, xd, Wd, bd, K, **kw)
    plan.set_option(_native.OPT_QSTRIP_IMAGE, IMG_ON)
    y_on2, _ = _native.cheb_forward(plan, xd, Wd, bd, K, **kw)  # (eager: rebuilds the image)
    assert torch.equal(y_on, y_off) and torch.equal(y_on, y_on2)
    torch.cuda.synchronize()
    out = torch.zeros_like(y_on)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            _native.cheb_forward(plan, xd, Wd, bd, K, out=out, **kw)
    torch.cuda.current_stream().wait_stream(side)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, y_on)


def test_the_image_itself(grid64):
    """Three strips of the nside-64 plan (the first, one that crosses a base-pixel border, the last): the image against a numpy
    gather from the plan's ELL through dsph_plan_strip_rows -- direction d of pixel (x, y) is the entry of L~ on the row of pixel
    (x + dx_d, y + dy_d) of the strip's plane -- on every pixel whose row of L~ an output needs (up to three pixels around the
    rectangle: the halo's outermost ring is read, its rows of L~ feed nothing).  Exact: doubling a float is exact."""
    cols, vals = grid64
    plan = _plan(cols, vals)
    rec = plan.strip_pairs(K)
    nside2 = 64 * 64

    def plane_rows(s, xs, ys):
        X, Y = np.meshgrid(xs, ys, indexing="ij")
        return plan.strip_rows(K, s, X.ravel(), Y.ravel()).reshape(X.shape)

    crossing = None
    for s in range(rec.shape[0]):
        r = rec[s]
        rows = plane_rows(s, np.arange(int(r[0]), int(r[0]) + int(r[2])), np.arange(int(r[6]), int(r[7])))
        if np.unique(rows // nside2).size > 1:
            crossing = s
            break
    assert crossing is not None, "no strip of the nside-64 plan crosses a base-pixel border"
    for s in (0, crossing, rec.shape[0] - 1):
        r = rec[s]
        xs0, xlo, xhi, ylo, yhi = int(r[4]), int(r[8]), int(r[9]), int(r[10]), int(r[11])
        ys = np.arange(ylo - 1, yhi + 7)
        for basis, factor in ((_native.BASIS_CHEBYSHEV, 2.0), (_native.BASIS_MONOMIAL, 1.0)):
            img = plan.strip_image(s, basis=basis)
            assert img.shape == (ys.size, 9, 16, 4)
            xcol = np.clip(xs0 + np.arange(64), xlo, xhi)  # column 4 p + t of the strip
            rows = plane_rows(s, xcol, ys)  # [64, rows]
            want = np.zeros((ys.size, 9, 64), np.float32)
            for v in range(9):
                dx, dy = (0, 0) if v == 0 else (_DX[v - 1], _DY[v - 1])
                nb = plane_rows(s, np.clip(xcol + dx, xlo, xhi), np.clip(ys + dy, ylo - 1, yhi + 6))
                hit = cols[rows] == nb[..., None]  # [64, rows, W]
                want[:, v, :] = (np.where(hit, vals[rows], 0.0).sum(axis=-1) * factor).T.astype(np.float32)
            got = img.reshape(ys.size, 9, 64)
            inner_x = (xs0 + np.arange(64) >= xlo + 1) & (xs0 + np.arange(64) <= xhi - 1)
            inner_y = (ys >= ylo + 1) & (ys <= yhi - 1)
            sel = np.ix_(inner_y, np.arange(9), inner_x)
            assert np.array_equal(got[sel], want[sel]), f"strip {s}, basis {basis}: image differs from the ELL"
            assert np.isfinite(got).all()
