"""CPU tests of the device build of HealpySmoothing's kernel table: the ``build`` keyword, the binding, the argument checks that run
before the library loads, the validity rule itself, ``healpix.transpose_table`` against the scipy route, and the completion and
assembly of ``healpix.gauss_table_device`` behind brute-force stand-ins for the two kernels.  No kernel runs without a GPU."""

import ctypes

import numpy as np
import pytest
import torch

import smoothing_build_ref as sb
from deepsphere import _native, healpix
from deepsphere.healpy_layers import HealpySmoothing


def test_build_keyword_is_checked():
    with pytest.raises(ValueError, match="elsewhere"):
        HealpySmoothing(4, np.arange(192), sigma=600.0, build="elsewhere")
    host = HealpySmoothing(4, np.arange(192), sigma=600.0, build="host")
    assert host.build_mode == "host" and host.completed == 0
    with pytest.raises(NotImplementedError):
        HealpySmoothing(4, np.arange(192), nest=False, sigma=600.0, build="device")


def test_device_build_without_a_gpu_raises_what_require_gpu_raises(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError) as want:
        _native.require_gpu()
    with pytest.raises(RuntimeError) as got:
        HealpySmoothing(4, np.arange(192), sigma=600.0, build="device")
    assert str(got.value) == str(want.value)


def test_entry_points_are_declared_in_the_binding():
    res, args = _native.SIGNATURES["dsph_healpix_disc_count"]
    assert res is ctypes.c_int and len(args) == 9 and args[1] is ctypes.c_double
    res, args = _native.SIGNATURES["dsph_healpix_gauss_table"]
    assert res is ctypes.c_int and len(args) == 13 and args[2] is ctypes.c_double and args[3] is ctypes.c_double
    assert _native.DISC_MAX_W >= 512 and _native.DISC_MAX_NSIDE == 8192
    lib = _native.lib()  # (every declared symbol is looked up on load)
    assert lib.dsph_healpix_disc_count is not None and lib.dsph_healpix_gauss_table is not None


def test_bad_arguments_are_refused_before_the_library_loads(monkeypatch):
    def no_lib():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_native, "lib", no_lib)
    monkeypatch.setattr(_native, "require_gpu", no_lib)
    idx = torch.arange(10, dtype=torch.int64)
    lut = torch.full((192,), -1, dtype=torch.int32)
    for nside in (3, 0, 16384):
        with pytest.raises(ValueError, match="nside"):
            _native.healpix_disc_count(nside, 0.1)
        with pytest.raises(ValueError, match="nside"):
            _native.healpix_gauss_table(nside, 8, 0.1, 0.3)
    with pytest.raises(ValueError, match="come together"):
        _native.healpix_disc_count(4, 0.1, indices=idx)
    with pytest.raises(ValueError, match="come together"):
        _native.healpix_gauss_table(4, 8, 0.1, 0.3, lut=lut)
    with pytest.raises(ValueError, match="int64"):
        _native.healpix_disc_count(4, 0.1, indices=idx.to(torch.int32), lut=lut)
    with pytest.raises(ValueError, match="lut"):
        _native.healpix_gauss_table(4, 8, 0.1, 0.3, indices=idx, lut=lut[:100].contiguous())
    for r2 in (-0.1, 4.5, float("nan")):
        with pytest.raises(ValueError, match="r2"):
            _native.healpix_disc_count(4, r2)
    with pytest.raises(ValueError, match=str(_native.DISC_MAX_W)):
        _native.healpix_gauss_table(16, _native.DISC_MAX_W + 1, 0.1, 0.3)
    with pytest.raises(ValueError, match="W = 0"):
        _native.healpix_gauss_table(4, 0, 0.1, 0.3)
    with pytest.raises(ValueError, match="M >= W"):
        _native.healpix_gauss_table(4, 11, 0.1, 0.3, indices=idx, lut=lut)
    for sigma, rho in ((0.0, 0.3), (0.1, 0.0), (0.1, 3.5)):
        with pytest.raises(ValueError, match="sigma_rad"):
            _native.healpix_gauss_table(4, 8, sigma, rho)
    with pytest.raises(ValueError, match="HIP device"):  # (a CPU tensor: still before the library)
        _native.healpix_disc_count(4, 0.1, indices=idx, lut=lut)
    with pytest.raises(ValueError, match="HIP device"):
        _native.healpix_gauss_table(4, 8, 0.1, 0.3, indices=idx, lut=lut)


@pytest.fixture(scope="module")
def n4():
    b = sb.brute(4, "full", 1.0, 3)
    return b, sb.brute_rows(b)


def test_validity_rule_accepts_brute_force_and_the_host_table(n4):
    b, (cols, vals, _) = n4
    assert b.W == 27 and sb.table_errors(b, cols, vals) == []
    layer = HealpySmoothing(4, np.arange(192), sigma=b.sigma_rad, arcmin=False)
    assert layer.max_neighbors == b.W and sb.table_errors(b, layer.cols.numpy(), layer.vals.numpy()) == []
    assert sb.table_errors(b, cols[5:9], vals[5:9], rows=np.arange(5, 9)) == []
    assert sb.table_errors_tree(4, None, b.sigma_rad, cols, vals, np.arange(192)) == []


def test_validity_rule_rejects_broken_rows(n4):
    b, (cols, vals, raw) = n4
    m = 17
    nearest = int(np.argsort(b.theta[m])[1])  # the nearest other pixel: far inside d_W
    far = int(np.argmax(b.theta[m]))

    def broken(fn):
        c, v = cols.copy(), vals.copy()
        fn(c, v)
        return sb.table_errors(b, c, v), sb.table_errors_tree(4, None, b.sigma_rad, c, v, np.arange(192))

    def drop_near(c, v):  # the antipode in place of a near pixel, the row sorted again
        row = np.where(c[m] == nearest, far, c[m])
        c[m] = np.sort(row)

    for errs in broken(drop_near):
        assert any("leave" in e and "nearer" in e for e in errs) and any("beyond" in e for e in errs)

    def repeat(c, v):
        c[m, 3] = c[m, 2]

    errs, errs_tree = broken(repeat)
    assert any("twice" in e for e in errs) and any("ascend" in e for e in errs_tree)

    def unsort(c, v):
        c[m, [2, 3]] = c[m, [3, 2]]
        v[m, [2, 3]] = v[m, [3, 2]]

    errs, errs_tree = broken(unsort)
    assert any("ascend" in e for e in errs) and any("ascend" in e for e in errs_tree)

    def raw_values(c, v):
        v[m] = raw[m]

    for errs in broken(raw_values):
        assert any("vals off" in e for e in errs) and any("sums to" in e for e in errs)


@pytest.mark.parametrize("nside,indices", [(4, np.arange(192)), (8, healpix.cap_indices(8))], ids=["n4_full", "n8_cap"])
def test_transpose_table_equals_the_scipy_route(nside, indices):
    layer = HealpySmoothing(nside, indices, sigma=1.0 * sb.res(nside), arcmin=False)
    want_c, want_v = layer._transposed_tables(torch.device("cpu"))
    got_c, got_v = healpix.transpose_table(layer.cols, layer.vals)
    assert got_c.dtype == torch.int32 and got_v.dtype == torch.float32
    assert torch.equal(got_c, want_c) and torch.equal(got_v.view(torch.int32), want_v.view(torch.int32))


def test_transpose_table_drops_explicit_zeros():
    layer = HealpySmoothing(4, np.arange(192), sigma=1.0 * sb.res(4), arcmin=False)
    cols, vals = layer.cols.clone(), layer.vals.clone()
    vals[3, 5] = 0.0
    vals[100] = 0.0  # a whole row: its pixel then feeds nothing
    vals[:, 0] = torch.where(cols[:, 0] == 7, torch.zeros(()), vals[:, 0])
    want_c, want_v = sb.scipy_transposed(cols.numpy(), vals.numpy())
    got_c, got_v = healpix.transpose_table(cols, vals)
    assert np.array_equal(got_c.numpy(), want_c) and np.array_equal(got_v.numpy().view(np.int32), want_v.view(np.int32))
    zero_c, zero_v = healpix.transpose_table(cols, torch.zeros_like(vals))
    assert zero_c.shape == (192, 1) and torch.equal(zero_c[:, 0], torch.arange(192, dtype=torch.int32)) and not bool(zero_v.any())


@pytest.mark.parametrize("which,nside,flag_count,flag_table,want", [
    ("full", 4, [], [], 0),
    ("full", 4, [3, 50], [50, 60, 191], 4),
    ("cap16", 16, list(range(0, 1152, 7)), list(range(0, 1152, 5)), None),
    ("cap16", 16, [0], [], 1),
])
def test_gauss_table_device_completes_flagged_rows(monkeypatch, which, nside, flag_count, flag_table, want):
    b = sb.brute(nside, which, 1.5 if which == "cap16" else 1.0, 3)
    fake = sb.FakeNative(b, flag_count, flag_table)
    monkeypatch.setattr(_native, "healpix_disc_count", fake.healpix_disc_count)
    monkeypatch.setattr(_native, "healpix_gauss_table", fake.healpix_gauss_table)
    cols, vals, raw, W, completed = healpix.gauss_table_device(nside, b.indices, b.sigma_rad, 3, device="cpu", want_raw=True)
    assert fake.calls == ["count", "table"]
    assert W == b.W and completed == (len(set(flag_count) | set(flag_table)) if want is None else want)
    assert cols.dtype == torch.int32 and vals.dtype == torch.float32 and raw.dtype == torch.float32
    assert sb.table_errors(b, cols.numpy(), vals.numpy()) == []
    # raw: the values before normalisation, on the same columns
    r = raw.numpy()
    np.testing.assert_allclose(r, np.take_along_axis(b.kern, cols.numpy().astype(np.int64), axis=1), rtol=1e-6)
    np.testing.assert_array_equal((r / r.sum(axis=1, dtype=np.float64, keepdims=True)).astype(np.float32), vals.numpy())
    assert healpix.gauss_table_device(nside, b.indices, b.sigma_rad, 3, device="cpu")[2] is None


def test_gauss_table_device_rows_follow_the_order_of_indices(monkeypatch):
    b = sb.brute(4, "full", 1.0, 3)
    perm = np.random.default_rng(2).permutation(192)
    shuffled = sb.Brute(4, perm, b.sigma_rad, 3)
    fake = sb.FakeNative(shuffled, [1], [2])
    monkeypatch.setattr(_native, "healpix_disc_count", fake.healpix_disc_count)
    monkeypatch.setattr(_native, "healpix_gauss_table", fake.healpix_gauss_table)
    cols, vals, _, W, completed = healpix.gauss_table_device(4, perm, b.sigma_rad, 3, device="cpu")
    assert W == b.W and completed == 2 and sb.table_errors(shuffled, cols.numpy(), vals.numpy()) == []
    with pytest.raises(ValueError, match="unique"):
        healpix.gauss_table_device(4, [1, 2, 2], b.sigma_rad, 3, device="cpu")


def test_rows_above_the_cap_name_the_cap_and_the_host_build(monkeypatch):
    b = sb.brute(4, "full", 1.0, 3)
    fake = sb.FakeNative(b)
    monkeypatch.setattr(_native, "healpix_disc_count", fake.healpix_disc_count)
    monkeypatch.setattr(_native, "healpix_gauss_table", fake.healpix_gauss_table)
    monkeypatch.setattr(_native, "DISC_MAX_W", 20)
    with pytest.raises(ValueError, match=r'up to 20 .*build="host"'):
        healpix.gauss_table_device(4, b.indices, b.sigma_rad, 3, device="cpu")
    assert fake.calls == ["count"]
