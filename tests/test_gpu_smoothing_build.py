"""GPU tests of the device build of HealpySmoothing's kernel table (``pytest -m gpu``): the kernels ``dsph_healpix_disc_count`` and
``dsph_healpix_gauss_table`` against brute force under the validity rule of tests/smoothing_build_ref.py, the completion behind
them (``healpix.gauss_table_device``), ``healpix.transpose_table`` on the device and ``HealpySmoothing(build="device")``.

No test asks for the host-built table: at a tied W-th neighbour either member of the tie is right.  The kernels write into
sentinel-guarded buffers.  sigma is given in pixel resolutions (``sb.res``)."""

import ctypes
import functools

import numpy as np
import pytest
import torch

import smoothing_build_ref as sb
import smoothing_ref as ref
from deepsphere import _native, healpix
from deepsphere.healpy_layers import HealpySmoothing

pytestmark = pytest.mark.gpu


def pixel_set(nside, which):
    if which == "full":
        return None, None
    return healpix._device_lut(nside, sb.SETS[which](nside), torch.device("cuda"))


def launch(nside, which, sigma_rad, rho, W):
    """Both kernels on one set, into guarded buffers: -> (count, count ok, cols, vals, raw, ok) numpy."""
    M = sb.SETS[which](nside).shape[0]
    ps = pixel_set(nside, which)
    dev = "cuda" if which == "full" else None  # (a set brings its device along)
    gc = sb.Guarded([(torch.int32, (M,)), (torch.uint8, (M,))])
    out = _native.healpix_disc_count(nside, sb.chord2(rho), *ps, device=dev, out=gc.out)
    torch.cuda.synchronize()
    assert out[0].data_ptr() == gc.out[0].data_ptr()
    gc.check(f"disc_count nside {nside} {which}")
    gt = sb.Guarded([(torch.int32, (M, W)), (torch.float32, (M, W)), (torch.float32, (M, W)), (torch.uint8, (M,))])
    out = _native.healpix_gauss_table(nside, W, sigma_rad, rho, *ps, device=dev, want_raw=True, out=gt.out)
    torch.cuda.synchronize()
    assert out[0].data_ptr() == gt.out[0].data_ptr()
    gt.check(f"gauss_table nside {nside} {which}")
    return tuple(t.cpu().numpy() for t in gc.out + gt.out)


@functools.lru_cache(maxsize=None)
def run_kernels(nside, which, f, n_sigma):
    """... at the brute-force W of the case, computed once per process and never written."""
    b = sb.brute(nside, which, f, n_sigma)
    return launch(nside, which, b.sigma_rad, b.rho, b.W)


# ---- the full sky ------------------------------------------------------------------------------------------------------------------
FULL_CASES = [(8, 1.0, 3, 29), (8, 1.5, 3, 64), (16, 1.0, 3, 30), (16, 1.5, 3, 66), (16, 2.0, 2, 52), (16, 3.0, 3, 252), (16, 4.0, 3, 436),
              (4, 1.0, 3, 27)]


@pytest.mark.parametrize("nside,f,n_sigma,W", FULL_CASES)
def test_full_sky_counts_and_tables(nside, f, n_sigma, W):
    b = sb.brute(nside, "full", f, n_sigma)
    assert b.W == W and b.rho <= np.pi / 4
    count, okc, cols, vals, raw, ok = run_kernels(nside, "full", f, n_sigma)
    assert okc.all() and ok.all(), f"{int((okc == 0).sum())} counts and {int((ok == 0).sum())} rows of a full sky flagged"
    assert np.array_equal(count, b.counts) and int(count.max()) == W
    assert sb.table_errors(b, cols, vals) == []
    np.testing.assert_array_equal((raw / raw.sum(axis=1, dtype=np.float64, keepdims=True)).astype(np.float32), vals)
    dc, dv, dr, dW, completed = healpix.gauss_table_device(nside, b.indices, b.sigma_rad, n_sigma, device="cuda")
    assert dW == W and completed == 0 and dr is None and dc.is_cuda
    assert np.array_equal(dc.cpu().numpy(), cols) and np.array_equal(dv.cpu().numpy(), vals)


# ---- discs that clip at both poles and take whole rings -----------------------------------------------------------------------------
WIDE_CASES = [(1, 1.0, 3, 11), (2, 1.5, 3, 40), (4, 1.5, 3, 60), (4, 3.0, 3, 163), (8, 4.0, 3, 374)]


@pytest.mark.parametrize("nside,f,n_sigma,W", WIDE_CASES)
def test_wide_discs(nside, f, n_sigma, W):
    b = sb.brute(nside, "full", f, n_sigma)
    assert b.W == W
    count, okc, cols, vals, raw, ok = run_kernels(nside, "full", f, n_sigma)
    print(f"nside {nside} sigma {f} res: radius {np.degrees(b.rho):.0f} deg, {int((okc == 0).sum())} counts, {int((ok == 0).sum())} rows flagged")
    good = np.nonzero(okc == 1)[0]
    assert np.array_equal(count[good], b.counts[good])
    good = np.nonzero(ok == 1)[0]
    assert sb.table_errors(b, cols[good], vals[good], rows=good) == []
    dc, dv, _, dW, completed = healpix.gauss_table_device(nside, b.indices, b.sigma_rad, n_sigma, device="cuda")
    assert dW == W and completed == int(((okc == 0) | (ok == 0)).sum())
    assert sb.table_errors(b, dc.cpu().numpy(), dv.cpu().numpy()) == []


# ---- every face border --------------------------------------------------------------------------------------------------------------
def test_all_faces_against_the_tree():
    from scipy.spatial import cKDTree

    nside, sigma = 64, 1.5 * sb.res(64)
    rho = 3 * sigma
    vec = healpix.pix2vec(nside)
    lens = cKDTree(vec).query_ball_point(vec, 2.0 * np.sin(0.5 * rho), return_length=True)
    W = int(lens.max())
    count, okc, cols, vals, raw, ok = launch(nside, "full", sigma, rho, W)
    assert okc.all() and ok.all()
    assert np.array_equal(count, lens)
    assert sb.table_errors_tree(nside, None, sigma, cols, vals, np.arange(12 * nside * nside)) == []


# ---- partial sky ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nside,which", [(16, "cap16"), (32, "ragged32")])
def test_partial_sky(nside, which):
    b = sb.brute(nside, which, 1.5, 3)
    ind, W = b.indices, b.W
    assert ind.shape[0] == {"cap16": 1152, "ragged32": 3680}[which]
    if which == "ragged32":
        assert W == 65
    count, okc, cols, vals, raw, ok = run_kernels(nside, which, 1.5, 3)
    good = np.nonzero(okc == 1)[0]
    assert np.array_equal(count[good], b.counts[good])
    good = np.nonzero(ok == 1)[0]
    assert sb.table_errors(b, cols[good], vals[good], rows=good) == []
    # a row whose W nearest in the set are its W nearest on the whole sphere is one the kernel must have guaranteed
    allvec = healpix.pix2vec(nside)
    vec = allvec[ind]
    dk_sky = np.empty(ind.shape[0])
    for a in range(0, ind.shape[0], 512):
        Ds = ((allvec[None, :, :] - vec[a:a + 512, None, :]) ** 2).sum(axis=2)
        dk_sky[a:a + 512] = np.sqrt(np.partition(Ds, W - 1, axis=1)[:, W - 1])
    dk_set = 2.0 * np.sin(0.5 * b.d_k)
    interior = dk_set <= dk_sky * (1 + sb.EPS)
    print(f"{which}: W {W}, {int(interior.sum())} interior rows, {int((ok == 0).sum())} rows flagged")
    assert interior.sum() > 0 and ok[interior].all(), f"{int((ok[interior] == 0).sum())} interior rows flagged"
    if which == "ragged32":
        assert (ok == 0).any()  # ... so the host completion below runs
    dc, dv, dr, dW, completed = healpix.gauss_table_device(nside, ind, b.sigma_rad, 3, device="cuda", want_raw=True)
    assert dW == W and completed == int(((okc == 0) | (ok == 0)).sum()) and completed >= int((ok == 0).sum())
    if not (okc == 0).any():
        assert completed == int((ok == 0).sum())
    dc, dv, dr = dc.cpu().numpy(), dv.cpu().numpy(), dr.cpu().numpy()
    assert sb.table_errors(b, dc, dv) == []
    np.testing.assert_array_equal((dr / dr.sum(axis=1, dtype=np.float64, keepdims=True)).astype(np.float32), dv)


# ---- determinism ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nside,which,f", [(16, "full", 1.5), (32, "ragged32", 1.5), (16, "full", 4.0)])
def test_two_runs_give_identical_bytes(nside, which, f):
    b = sb.brute(nside, which, f, 3)
    first = run_kernels(nside, which, f, 3)
    again = launch(nside, which, b.sigma_rad, b.rho, b.W)
    for a, c in zip(first, again):
        assert a.tobytes() == c.tobytes()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_their_code_without_a_launch():
    lib = _native.lib()
    BADARG, UNSUPPORTED = -1, -3
    M = 192
    g = sb.Guarded([(torch.int32, (M, 8)), (torch.float32, (M, 8)), (torch.uint8, (M,)), (torch.int32, (M,))])
    cols, vals, ok, count = g.out
    before = [t.clone() for t in (cols, ok, count)]
    idx = torch.arange(M, dtype=torch.int64, device="cuda")
    p, null, stream = _native._ptr, ctypes.c_void_p(), _native._stream_ptr(torch.device("cuda", 0))

    def table(nside=4, W=8, indices=null, lut=null, m=M, c=None, v=None, o=None):
        return lib.dsph_healpix_gauss_table(nside, W, 0.2, 0.6, indices, lut, m, p(cols) if c is None else c, p(vals) if v is None else v,
                                            null, p(ok) if o is None else o, 0, stream)

    def counts(nside=4, indices=null, lut=null, m=M, c=None, o=None):
        return lib.dsph_healpix_disc_count(nside, 0.3, indices, lut, m, p(count) if c is None else c, p(ok) if o is None else o, 0, stream)

    assert table(W=_native.DISC_MAX_W + 1, nside=16, m=3072) == UNSUPPORTED and str(_native.DISC_MAX_W) in _native.last_error()
    assert table(nside=3, m=108) == BADARG and "power of two" in _native.last_error()
    assert counts(nside=3, m=108) == BADARG
    assert table(nside=16384, m=M) == UNSUPPORTED and counts(nside=16384, m=M) == UNSUPPORTED
    assert table(indices=p(idx)) == BADARG and "come together" in _native.last_error()
    assert counts(indices=p(idx)) == BADARG
    assert table(c=null) == BADARG and table(v=null) == BADARG and table(o=null) == BADARG and "NULL" in _native.last_error()
    assert counts(c=null) == BADARG and counts(o=null) == BADARG
    assert table(W=0) == BADARG and table(m=100) == BADARG
    torch.cuda.synchronize()
    for t, was in zip((cols, ok, count), before):
        assert torch.equal(t, was)
    # a window beyond the LDS budget: a 60 degree disc at nside 64 holds some 12,000 pixels
    big = torch.empty((49152, 8), dtype=torch.int32, device="cuda")
    rc = lib.dsph_healpix_gauss_table(64, 8, 0.3, 1.05, null, null, 49152, p(big), p(big.view(torch.float32)), null,
                                      p(torch.empty(49152, dtype=torch.uint8, device="cuda")), 0, stream)
    assert rc == UNSUPPORTED and "candidates" in _native.last_error()
    with pytest.raises(ValueError, match='build="host"'):  # W = 12,000 or so
        HealpySmoothing(64, np.arange(49152), sigma=0.35, arcmin=False, build="device")


def test_a_pixel_outside_the_sphere_is_flagged_and_reads_nothing():
    nside, W = 8, 29
    sigma = sb.res(nside)
    ind = np.arange(100, 400, dtype=np.int64)
    ti, lut = healpix._device_lut(nside, ind, torch.device("cuda"))
    ti = ti.clone()
    ti[[7, 250]] = torch.tensor([768, -5], device="cuda")
    cols, vals, raw, ok = _native.healpix_gauss_table(nside, W, sigma, 3 * sigma, ti, lut, want_raw=True)
    count, okc = _native.healpix_disc_count(nside, sb.chord2(3 * sigma), ti, lut)
    torch.cuda.synchronize()
    for r in (7, 250):
        assert int(ok[r]) == 0 and int(okc[r]) == 0 and bool((cols[r] == -1).all()) and not bool(vals[r].any())


# ---- the layer -----------------------------------------------------------------------------------------------------------------------
def bound(W, r, scale):
    return 2 * r * (W + 8) * 2.0**-24 * scale  # (tests/test_gpu_smoothing.py)


@pytest.mark.parametrize("which", ["full", "cap16"])
def test_layer_built_on_the_device(which):
    nside = 16
    ind = sb.SETS[which](nside)
    M, C = ind.shape[0], 3
    rng = np.random.default_rng(11)
    reps = None if which == "full" else [0, 1, 3]
    mask = None if which == "full" else rng.random(M) < 0.7
    layer = HealpySmoothing(nside, ind, sigma=1.5 * sb.res(nside), arcmin=False, mask=mask, per_channel_repetitions=reps, build="device")
    b = sb.brute(nside, which, 1.5, 3)
    assert layer.build_mode == "device" and layer.max_neighbors == b.W and layer.cols.is_cuda and layer.vals.is_cuda
    assert layer.cols.dtype == torch.int32 and layer.vals.dtype == torch.float32 and "cols" not in layer.state_dict()
    cols, vals = layer.cols.cpu().numpy(), layer.vals.cpu().numpy()
    assert sb.table_errors(b, cols, vals) == []
    assert layer.completed == (0 if which == "full" else int((run_kernels(nside, which, 1.5, 3)[5] == 0).sum()))
    x = rng.standard_normal((2, M, C)).astype(np.float32)
    g = rng.standard_normal((2, M, C)).astype(np.float32)
    xt = torch.as_tensor(x).cuda().requires_grad_(True)
    y = layer(xt)
    r = ref.n_passes(reps)
    err, tol = np.abs(y.detach().cpu().numpy() - ref.apply(cols, vals, x, reps, mask)).max(), bound(b.W, r, np.abs(x).max())
    print(f"{which}: forward err {err:.3e} bound {tol:.3e}")
    assert err <= tol
    y.backward(torch.as_tensor(g).cuda())
    torch.cuda.synchronize()
    colsT, valsT = layer._tables_T
    assert colsT.is_cuda and valsT.is_cuda
    want_c, want_v = sb.scipy_transposed(cols, vals)
    assert np.array_equal(colsT.cpu().numpy(), want_c) and np.array_equal(valsT.cpu().numpy().view(np.int32), want_v.view(np.int32))
    K = ref.dense(cols, vals)
    want = ref.apply_transposed(K, g, reps, mask)
    WT, S = colsT.shape[1], K.sum(axis=0).max()
    err, tol = np.abs(xt.grad.cpu().numpy() - want).max(), bound(WT, r, np.abs(g).max() * max(S, 1.0) ** r)
    print(f"{which}: input gradient err {err:.3e} bound {tol:.3e} (WT {WT}, S {S:.3f})")
    assert err <= tol


def test_data_path_round_trip_between_the_builds(tmp_path, monkeypatch):
    nside, ind = 16, sb.cap16()
    sigma = 1.5 * sb.res(nside)
    dev = HealpySmoothing(nside, ind, sigma=sigma, arcmin=False, data_path=str(tmp_path), build="device")
    files = sorted(p.name for p in tmp_path.iterdir())
    assert files == [f"ind_coo{dev.file_label}.npy", f"val_coo{dev.file_label}.npy"]
    monkeypatch.setattr(HealpySmoothing, "_build_tree", lambda self: pytest.fail("the stored kernel was not loaded"))
    monkeypatch.setattr(healpix, "gauss_table_device", lambda *a, **k: pytest.fail("the stored kernel was not loaded"))
    host = HealpySmoothing(nside, ind, sigma=sigma, arcmin=False, data_path=str(tmp_path), build="host")
    assert host.max_neighbors == dev.max_neighbors and not host.cols.is_cuda
    assert np.array_equal(host.cols.numpy(), dev.cols.cpu().numpy())
    np.testing.assert_allclose(host.vals.numpy(), dev.vals.cpu().numpy(), rtol=1e-6, atol=0)
    again = HealpySmoothing(nside, ind, sigma=sigma, arcmin=False, data_path=str(tmp_path), build="device")  # loads, whatever build says
    assert np.array_equal(again.cols.cpu().numpy(), host.cols.numpy()) and again.build_mode == "device"


# ---- one larger build ------------------------------------------------------------------------------------------------------------------
def test_nside_128_build():
    from scipy.spatial import cKDTree

    nside, M = 128, 196608
    sigma = 1.5 * sb.res(nside)
    rho = 3 * sigma
    ps = (None, None)
    count, okc = _native.healpix_disc_count(nside, sb.chord2(rho), *ps, device="cuda")
    W = int(count.max())
    g = sb.Guarded([(torch.int32, (M, W)), (torch.float32, (M, W)), (torch.uint8, (M,))])
    cols, vals, ok = g.out
    _native.healpix_gauss_table(nside, W, sigma, rho, *ps, device="cuda", out=(cols, vals, None, ok))
    torch.cuda.synchronize()
    g.check("gauss_table nside 128")
    assert bool(okc.all()) and bool(ok.all())
    assert float((vals.to(torch.float64).sum(dim=1) - 1.0).abs().max()) <= W * 2.0**-24
    rows = np.sort(np.random.default_rng(7).choice(M, size=4096, replace=False))
    vec = healpix.pix2vec(nside)
    lens = cKDTree(vec).query_ball_point(vec[rows], 2.0 * np.sin(0.5 * rho), return_length=True)
    assert np.array_equal(count.cpu().numpy()[rows], lens)
    assert sb.table_errors_tree(nside, None, sigma, cols.cpu().numpy(), vals.cpu().numpy(), rows) == []
