"""GPU tests of the harmonic-transform kernels (``dsph_sht_ring_analysis``, ``dsph_sht_legendre_analysis``,
``dsph_sht_legendre_synthesis``, ``dsph_sht_ring_synthesis``), of their compositions, of ``deepsphere.sht`` and of
``HealpyPowerSpectrum`` on them (``pytest -m gpu``).

The reference is the numpy transform of ``deepsphere.healpix`` (long-double Legendre recurrence, float64 sums), proven on the CPU
in tests/test_sht_host.py; it is computed once per (nside, lmax) for the widest batch (tests/sht_ref.py) and sliced by the cases.

Tolerances -- derived from the arithmetic, not measured.  The kernels work in float64: a term of the recurrence carries about
(l - m) 2^-53 relative error, |lambda_lm| <= sqrt((2 l + 1) / 4 pi), a twiddle is at most 15 rotations (4 roundings each) from an
exact sincospi, and the maps are stored as float32.
  nside <= 32 (l <= 127, rings of at most 128 pixels):
    analysis (and its two stages)   1e-10 max|input|: a ring sum of <= 128 pixels with twiddles good to 1e-14 is within 2e-12 max|x|;
                                    a_lm = w sum_rings lambda F with w (4 nside - 1) sqrt(255 / 4 pi) <= 19 and lambda good to
                                    127 * 2^-53 = 1.4e-14 is within 3e-13 max|F_m|; the rest is summation order
    Legendre synthesis              1e-10 max|alm|: 128 terms of |lambda| <= 4.5 good to 1.4e-14: 8e-12 max|alm|
    synthesis to a map              2^-23 max|map|: the float32 store is within 2^-24 of the float64 value, which itself is good to 1e-10
  lmax = 3071 (nside 1024):         1e-8 max|F_m| for the Legendre analysis and 1e-8 max|alm| for the Legendre synthesis:
                                    3071 * 2^-53 = 3.4e-13 per term, 1500 * 1e-16 from sin^m theta, over <= 4095 rings or 3072 l
  spectra in float32                4 * 2^-24 max C_l
The gradient bounds are stated at their tests.

Outputs are NaN-filled views between sentinel bands (``large_map_ref.Guarded``); inputs are checksummed before and after."""

import numpy as np
import pytest
import torch

import large_map_ref as lm
import sht_ref as sr
from deepsphere import _native, healpix, sht
from deepsphere.healpy_layers import HealpyChebyshev, HealpyPowerSpectrum
from deepsphere.healpy_networks import HealpyGCNN
from helpers import offset_view

pytestmark = pytest.mark.gpu

TOL_A = 1e-10
TOL_MAP = 2.0 ** -23
TOL_BIG = 1e-8
TOL_CL = 4 * 2.0 ** -24


def fresh(a):
    """A writable C-ordered copy of a (slice of a) cached array."""
    return np.array(a, order="C")


def guarded(shape, dtype=torch.float32, misalign=0):
    return lm.Guarded(tuple(shape), device="cuda", misalign=misalign, dtype=dtype)


def checksum64(t):
    return int(torch.view_as_real(t).reshape(-1).view(torch.int64).sum()) if t.is_complex() else int(t.reshape(-1).view(torch.int64).sum())


def dev_sets(nside, ind):
    if ind is None:
        return None, None
    return healpix._device_lut(nside, ind, torch.device("cuda", torch.cuda.current_device()))


def run_analysis(nside, lmax, N, F, mis_x=0):
    """Both stages and the composition on base_maps[:N, :, :F] against the host: -> alm (device)."""
    x = fresh(sr.base_maps(nside)[:N, :, :F])
    xmax = float(np.abs(x).max())
    xd = offset_view(x, mis_x) if mis_x else torch.from_numpy(x).cuda()
    before = lm.checksum(xd)
    fm_ref, alm_ref = (sr.pick(a, N, F) for a in sr.analysis_reference(nside, lmax))
    what = f"nside {nside} lmax {lmax} N {N} F {F}"
    # stage 1
    g = guarded(_native.sht_fm_shape(nside, lmax, N, F), torch.float64)
    fm = _native.sht_ring_analysis(xd, nside, lmax, out=g.view)
    torch.cuda.synchronize()
    g.check(what)
    assert lm.checksum(xd) == before
    err = np.abs(sr.fm_to_numpy(fm) - fm_ref).max()
    print(f"{what}: ring analysis {err / xmax:.3e} max|x|")
    assert err <= TOL_A * xmax, (what, err)
    # stage 2, from the host's F_m
    fin = sr.fm_to_tensor(fm_ref, "cuda")
    fsum = checksum64(fin)
    ga = guarded((N, healpix.alm_size(lmax), F), torch.complex128)
    alm = _native.sht_legendre_analysis(fin, nside, lmax, N, F, out=ga.view)
    torch.cuda.synchronize()
    ga.check(what)
    assert checksum64(fin) == fsum
    err = np.abs(sr.columns(alm.cpu().numpy()) - alm_ref).max()
    print(f"{what}: Legendre analysis {err / max(np.abs(fm_ref).max(), 1e-300):.3e} max|F_m|")
    assert err <= TOL_A * np.abs(fm_ref).max(), (what, err)
    # the composition
    gc = guarded((N, healpix.alm_size(lmax), F), torch.complex128)
    alm = _native.sht_analysis(xd, nside, lmax, out=gc.view)
    torch.cuda.synchronize()
    gc.check(what)
    assert lm.checksum(xd) == before and alm.data_ptr() == gc.view.data_ptr()
    err = np.abs(sr.columns(alm.cpu().numpy()) - alm_ref).max()
    print(f"{what}: analysis {err / xmax:.3e} max|x|")
    assert err <= TOL_A * xmax, (what, err)
    return alm


def run_synthesis(nside, lmax, N, F, mis_y=0):
    a = fresh(sr.base_alm(lmax)[:N, :, :F])
    amax = float(np.abs(a).max())
    ad = torch.from_numpy(a).cuda()
    before = checksum64(ad)
    fm_ref, map_ref = (sr.pick(v, N, F) for v in sr.synthesis_reference(nside, lmax))
    what = f"nside {nside} lmax {lmax} N {N} F {F}"
    g = guarded(_native.sht_fm_shape(nside, lmax, N, F), torch.float64)
    fm = _native.sht_legendre_synthesis(ad, nside, out=g.view)
    torch.cuda.synchronize()
    g.check(what)
    assert checksum64(ad) == before
    err = np.abs(sr.fm_to_numpy(fm) - fm_ref).max()
    print(f"{what}: Legendre synthesis {err / amax:.3e} max|alm|")
    assert err <= TOL_A * amax, (what, err)
    fin = sr.fm_to_tensor(fm_ref, "cuda")
    fsum = checksum64(fin)
    mmax = float(np.abs(map_ref).max())
    gm = guarded((N, 12 * nside * nside, F), misalign=mis_y)
    y = _native.sht_ring_synthesis(fin, nside, lmax, N, F, out=gm.view)
    torch.cuda.synchronize()
    gm.check(what)
    assert checksum64(fin) == fsum
    err = np.abs(sr.columns(y.cpu().numpy().astype(np.float64)) - map_ref).max()
    print(f"{what}: ring synthesis {err / mmax:.3e} max|map|")
    assert err <= TOL_MAP * mmax, (what, err)
    gc = guarded((N, 12 * nside * nside, F), misalign=mis_y)
    y = _native.sht_synthesis(ad, nside, out=gc.view)
    torch.cuda.synchronize()
    gc.check(what)
    assert checksum64(ad) == before and y.data_ptr() == gc.view.data_ptr()
    err = np.abs(sr.columns(y.cpu().numpy().astype(np.float64)) - map_ref).max()
    print(f"{what}: synthesis {err / mmax:.3e} max|map|")
    assert err <= TOL_MAP * mmax, (what, err)
    return y


@pytest.mark.parametrize("nside,lmax", sr.GRID)
def test_analysis_against_the_host_reference(nside, lmax):
    for N in sr.NS:
        for F in sr.FS:
            run_analysis(nside, lmax, N, F)


@pytest.mark.parametrize("nside,lmax", sr.GRID)
def test_synthesis_against_the_host_reference(nside, lmax):
    for N in sr.NS:
        for F in sr.FS:
            run_synthesis(nside, lmax, N, F)


BIG_NSIDE, BIG_LMAX, BIG_MS = 1024, 3071, (0, 1, 1000, 1500, 2047, 3071)


def test_legendre_analysis_over_the_exponent_range():
    """nside 1024, lmax 3071, one column: F_m random in six columns of m, zero elsewhere.  lambda_mm of m = 1000 and 1500 starts
    hundreds of orders below float64 at the polar rings; a kernel on the plain recurrence is wrong from l ~ 2000 on."""
    nside, lmax = BIG_NSIDE, BIG_LMAX
    R = 4 * nside - 1
    rng = np.random.default_rng(31)
    fm = torch.zeros(_native.sht_fm_shape(nside, lmax, 1, 1), dtype=torch.float64, device="cuda")
    w = 4.0 * np.pi / (12 * nside * nside)
    expect = {}
    for m in BIG_MS:
        col = rng.standard_normal(R) + 1j * rng.standard_normal(R)
        fm[m, :, 0, :] = torch.view_as_real(torch.from_numpy(col)).cuda()
        expect[m] = w * (healpix.legendre_lambda(nside, m, lmax) @ col)
    fmax = float(fm.abs().max())
    ga = guarded((1, healpix.alm_size(lmax), 1), torch.complex128)
    alm = _native.sht_legendre_analysis(fm, nside, lmax, 1, 1, out=ga.view)
    torch.cuda.synchronize()
    ga.check("exponent range, analysis")
    got = alm.cpu().numpy()[0, :, 0]
    rest = np.ones(got.shape[0], dtype=bool)
    for m in BIG_MS:
        i0 = int(healpix.alm_index(lmax, m, m))
        err = np.abs(got[i0:i0 + lmax + 1 - m] - expect[m]).max()
        print(f"m {m}: {err / fmax:.3e} max|F_m|, max|a_lm| {np.abs(expect[m]).max():.3e}")
        assert np.isfinite(got[i0:i0 + lmax + 1 - m]).all() and err <= TOL_BIG * fmax, (m, err)
        rest[i0:i0 + lmax + 1 - m] = False
    assert np.all(got[rest] == 0), "a coefficient of an empty column of m is not exactly zero"


def test_legendre_synthesis_over_the_exponent_range():
    nside, lmax = BIG_NSIDE, BIG_LMAX
    rng = np.random.default_rng(32)
    alm = torch.zeros((1, healpix.alm_size(lmax), 1), dtype=torch.complex128, device="cuda")
    expect = {}
    for m in BIG_MS:
        i0 = int(healpix.alm_index(lmax, m, m))
        col = rng.standard_normal(lmax + 1 - m) + 1j * rng.standard_normal(lmax + 1 - m)
        alm[0, i0:i0 + lmax + 1 - m, 0] = torch.from_numpy(col).cuda()
        expect[m] = healpix.legendre_lambda(nside, m, lmax).T @ col
    amax = float(alm.abs().max())
    g = guarded(_native.sht_fm_shape(nside, lmax, 1, 1), torch.float64)
    fm = _native.sht_legendre_synthesis(alm, nside, out=g.view)
    torch.cuda.synchronize()
    g.check("exponent range, synthesis")
    for m in BIG_MS:
        got = torch.view_as_complex(fm[m, :, 0, :].contiguous()).cpu().numpy()
        err = np.abs(got - expect[m]).max()
        print(f"m {m}: {err / amax:.3e} max|alm|, max|F_m| {np.abs(expect[m]).max():.3e}")
        assert np.isfinite(got).all() and err <= TOL_BIG * amax, (m, err)
    keep = torch.ones(lmax + 1, dtype=torch.bool, device="cuda")
    keep[list(BIG_MS)] = False
    assert bool((fm[keep] == 0).all()), "F_m of an empty column of m is not exactly zero"


@pytest.mark.parametrize("nside", (8, 16))
@pytest.mark.parametrize("name", ("cap", "pair"))
def test_footprints_are_the_zero_filled_full_sky(nside, name):
    ind = sr.footprints(nside)[name]
    ti, lut = dev_sets(nside, ind)
    lmax, N, F = 3 * nside - 1, 2, 3
    npix = 12 * nside * nside
    x = torch.from_numpy(fresh(sr.base_maps(nside)[:N, ind, :F])).cuda()
    full = torch.zeros((N, npix, F), device="cuda")
    full[:, ti] = x
    ga = guarded((N, healpix.alm_size(lmax), F), torch.complex128)
    alm = _native.sht_analysis(x, nside, lmax, ti, lut, out=ga.view)
    ga.check(name)
    assert torch.equal(alm, _native.sht_analysis(full, nside, lmax))
    ref = sr.host_legendre_analysis(sr.host_fm(full.cpu().numpy(), nside, lmax), nside, lmax)
    assert np.abs(sr.columns(alm.cpu().numpy()) - ref).max() <= TOL_A * float(x.abs().max())
    # synthesis writes the footprint's rows, all of them and nothing else
    a = torch.from_numpy(fresh(sr.base_alm(lmax)[:N, :, :F])).cuda()
    gm = guarded((N, ind.size, F))
    y = _native.sht_synthesis(a, nside, ti, lut, out=gm.view)
    torch.cuda.synchronize()
    gm.check(name)
    assert bool(torch.isfinite(y).all()), "a row of the footprint was not written"
    assert torch.equal(y, _native.sht_synthesis(a, nside)[:, ti])


@pytest.mark.parametrize("F", (1, 2, 4, 16))
@pytest.mark.parametrize("mis", (1, 2))
def test_views_off_16_byte_alignment(F, mis):
    """Maps 4 and 8 bytes off 16-byte alignment, read (analysis) and written (synthesis)."""
    nside, lmax = 8, 23
    run_analysis(nside, lmax, 2, F, mis_x=mis)
    run_synthesis(nside, lmax, 2, F, mis_y=mis)


def small_reference(x, lmax):
    """nside 1: the host analysis of maps (N, 12, F) -> (N, nalm, F)."""
    return sr.uncolumns(sr.host_legendre_analysis(sr.host_fm(x, 1, lmax), 1, lmax), x.shape[0], x.shape[2])


def test_more_columns_than_a_scratch_chunk():
    """N = 4,096 maps of F = 17 channels at nside 1: the compositions take them in several trips through one scratch array."""
    nside, lmax, N, F = 1, 3, 4096, 17
    assert N > _native.sht_chunk_maps(nside, lmax, F) and N % _native.sht_chunk_maps(nside, lmax, F) != 0
    x = torch.randn((N, 12, F), generator=torch.Generator().manual_seed(5))
    alm = _native.sht_analysis(x.cuda(), nside, lmax)
    ref = small_reference(x.numpy().astype(np.float64), lmax)
    assert np.abs(alm.cpu().numpy() - ref).max() <= TOL_A * float(x.abs().max())
    a = torch.from_numpy(ref).cuda()
    gm = guarded((N, 12, F))
    y = _native.sht_synthesis(a, nside, out=gm.view)
    torch.cuda.synchronize()
    gm.check("chunks")
    back = sr.uncolumns(sr.host_ring_synthesis(sr.host_legendre_synthesis(sr.columns(ref), nside, lmax), nside), N, F)
    assert np.abs(y.cpu().numpy() - back).max() <= TOL_MAP * np.abs(back).max()


def test_one_more_map_than_the_grid():
    """The four stages with 8 * 4096 + 1 columns at nside 1: one more than the column blocks of a grid cover in one trip."""
    nside, lmax, F = 1, 3, 1
    N = 8 * 4096 + 1
    x = torch.randn((N, 12, F), generator=torch.Generator().manual_seed(6))
    x64 = x.numpy().astype(np.float64)
    fm_ref = sr.host_fm(x64, nside, lmax)
    fm = _native.sht_ring_analysis(x.cuda(), nside, lmax)
    assert np.abs(sr.fm_to_numpy(fm) - fm_ref).max() <= TOL_A * float(x.abs().max())
    alm_ref = sr.host_legendre_analysis(fm_ref, nside, lmax)
    alm = _native.sht_legendre_analysis(sr.fm_to_tensor(fm_ref, "cuda"), nside, lmax, N, F)
    assert np.abs(sr.columns(alm.cpu().numpy()) - alm_ref).max() <= TOL_A * np.abs(fm_ref).max()
    fs_ref = sr.host_legendre_synthesis(alm_ref, nside, lmax)
    fs = _native.sht_legendre_synthesis(torch.from_numpy(sr.uncolumns(alm_ref, N, F)).cuda(), nside)
    assert np.abs(sr.fm_to_numpy(fs) - fs_ref).max() <= TOL_A * np.abs(alm_ref).max()
    map_ref = sr.host_ring_synthesis(fs_ref, nside)
    gm = guarded((N, 12, F))
    y = _native.sht_ring_synthesis(sr.fm_to_tensor(fs_ref, "cuda"), nside, lmax, N, F, out=gm.view)
    torch.cuda.synchronize()
    gm.check("grid")
    assert np.abs(sr.columns(y.cpu().numpy().astype(np.float64)) - map_ref).max() <= TOL_MAP * np.abs(map_ref).max()


def test_two_runs_are_bit_identical():
    nside, lmax, N, F = 16, 47, 2, 3
    x = torch.from_numpy(fresh(sr.base_maps(nside)[:N, :, :F])).cuda()
    a = torch.from_numpy(fresh(sr.base_alm(lmax)[:N, :, :F])).cuda()
    assert torch.equal(torch.view_as_real(_native.sht_analysis(x, nside, lmax)), torch.view_as_real(_native.sht_analysis(x, nside, lmax)))
    assert torch.equal(_native.sht_synthesis(a, nside), _native.sht_synthesis(a, nside))


def test_empty_and_refused_inputs():
    nside, lmax = 4, 11
    x0 = torch.zeros((0, 192, 3), device="cuda")
    assert tuple(_native.sht_analysis(x0, nside, lmax).shape) == (0, healpix.alm_size(lmax), 3)
    assert tuple(_native.sht_synthesis(torch.zeros((0, healpix.alm_size(lmax), 3), dtype=torch.complex128, device="cuda"), nside).shape) == (0, 192, 3)
    assert tuple(sht.anafast(x0, nside).shape) == (0, 12, 3)
    # out= sharing memory with the input
    nalm = healpix.alm_size(lmax)
    buf = torch.zeros(max(192 * 3, 4 * nalm * 3) + 8, dtype=torch.float32, device="cuda")
    x = buf[:192 * 3].view(1, 192, 3)
    alias = buf[:4 * nalm * 3].view(torch.complex128).view(1, nalm, 3)
    with pytest.raises(ValueError, match="shares memory"):
        _native.sht_analysis(x, nside, lmax, out=alias)
    with pytest.raises(ValueError, match="shares memory"):
        _native.sht_synthesis(alias, nside, out=x)
    # a CPU out= for HIP input
    with pytest.raises(ValueError, match="out must be"):
        _native.sht_analysis(torch.zeros((1, 192, 3), device="cuda"), nside, lmax, out=torch.zeros((1, nalm, 3), dtype=torch.complex128))
    with pytest.raises(ValueError, match="out must be"):
        _native.sht_synthesis(torch.zeros((1, nalm, 3), dtype=torch.complex128, device="cuda"), nside, out=torch.zeros((1, 192, 3)))


# ---- sht.py and HealpyPowerSpectrum ------------------------------------------------------------------------------------------------

def host_cl(x, nside, lmax, it, ind=None):
    """(N, M, F) float64 numpy -> (N, lmax + 1, F) by healpix.anafast on the zero-filled maps."""
    N, M, F = x.shape
    full = np.zeros((12 * nside * nside, N * F))
    full[np.arange(12 * nside * nside) if ind is None else ind] = sr.columns(x)
    return sr.uncolumns(healpix.anafast(full, lmax=lmax, iter=it), N, F)


@pytest.mark.parametrize("nside", (8, 16))
@pytest.mark.parametrize("it", (0, 1))
def test_power_spectrum_forward(nside, it):
    N, F = 2, 3
    lmax = 3 * nside - 1
    for ind in (None, sr.footprints(nside)["cap"]):
        x = fresh(sr.base_maps(nside)[:N, :, :F] if ind is None else sr.base_maps(nside)[:N, ind, :F])
        layer = HealpyPowerSpectrum(nside, indices=ind, iter=it)
        cl = layer(torch.from_numpy(x).cuda())
        assert cl.dtype == torch.float32 and tuple(cl.shape) == (N, lmax + 1, F)
        ref = host_cl(x.astype(np.float64), nside, lmax, it, ind)
        err = np.abs(cl.cpu().numpy() - ref).max()
        print(f"nside {nside} iter {it} {'full sky' if ind is None else 'cap'}: {err / ref.max():.3e} max C_l")
        assert err <= TOL_CL * ref.max()


@pytest.mark.parametrize("nside", (8, 16))
def test_power_spectrum_backward_is_one_synthesis(nside):
    """iter = 0: dx = w alm2map(b), b_lm = 2 gC_l a_lm / (2 l + 1), evaluated by the host reference in float64.  Bound: the
    device rounds the map to float32 once (2^-24 max|dx|; the weight is applied to the float64 coefficients), its a_lm are good to
    1e-10: 2^-23 max|dx|."""
    N, F = 2, 3
    lmax = 3 * nside - 1
    for ind in (None, sr.footprints(nside)["cap"]):
        x = fresh(sr.base_maps(nside)[:N, :, :F] if ind is None else sr.base_maps(nside)[:N, ind, :F])
        gc = torch.randn((N, lmax + 1, F), generator=torch.Generator().manual_seed(nside))
        xd = torch.from_numpy(x).cuda().requires_grad_(True)
        HealpyPowerSpectrum(nside, indices=ind)(xd).backward(gc.cuda())
        full = np.zeros((12 * nside * nside, N * F))
        full[np.arange(12 * nside * nside) if ind is None else ind] = sr.columns(x.astype(np.float64))
        a = healpix.map2alm(full, lmax=lmax, iter=0)
        ls = np.concatenate([np.arange(m, lmax + 1) for m in range(lmax + 1)])
        b = 2.0 * sr.columns(gc.numpy().astype(np.float64))[ls] * a / (2.0 * ls[:, None] + 1.0)
        dx = (4.0 * np.pi / (12 * nside * nside)) * healpix.alm2map(b, nside)
        dx = dx if ind is None else dx[ind]
        err = np.abs(sr.columns(xd.grad.cpu().numpy().astype(np.float64)) - dx).max()
        print(f"nside {nside} {'full sky' if ind is None else 'cap'}: {err / np.abs(dx).max():.3e} max|dx|")
        assert err <= 2.0 ** -23 * np.abs(dx).max()


@pytest.mark.parametrize("nside", (8, 16))
def test_power_spectrum_backward_with_an_iteration(nside):
    """iter = 1 against a central difference of the host reference along two random directions v.  map2alm with Jacobi steps is
    linear in the map, so L(x) = sum gC C_l(x) is a quadratic and the central difference with step h = 1 is exact but for the
    rounding of L in float64: 64 * 2^-53 max|L| / h at most.  The device gradient passes five float32 maps (two transposed analyses,
    a transposed synthesis' input, two sums of gradients), each within 2^-24 of values that stay below 2 max|dx|:
    |<dx, v> - dL| <= 16 * 2^-24 max|dx| sum|v| + 64 * 2^-53 max|L|."""
    N, F = 1, 2
    lmax = 3 * nside - 1
    x = fresh(sr.base_maps(nside)[:N, :, :F])
    gc = np.random.default_rng(nside).standard_normal((N, lmax + 1, F))
    xd = torch.from_numpy(x).cuda().requires_grad_(True)
    (HealpyPowerSpectrum(nside, iter=1)(xd).double() * torch.from_numpy(gc).cuda()).sum().backward()
    dx = xd.grad.cpu().numpy().astype(np.float64)

    def loss(v):
        return float((host_cl(v, nside, lmax, 1) * gc).sum())

    for seed in (1, 2):
        v = np.random.default_rng(100 + seed).standard_normal(x.shape)
        lp, lm_ = loss(x.astype(np.float64) + v), loss(x.astype(np.float64) - v)
        fd = 0.5 * (lp - lm_)
        got = float((dx * v).sum())
        bound = 16 * 2.0 ** -24 * np.abs(dx).max() * np.abs(v).sum() + 64 * 2.0 ** -53 * max(abs(lp), abs(lm_))
        print(f"nside {nside} direction {seed}: <dx, v> {got:.9e}, central difference {fd:.9e}, bound {bound:.3e}")
        assert abs(got - fd) <= bound


@pytest.mark.parametrize("nside", (4, 8))
def test_the_transforms_are_adjoint_on_the_device(nside):
    """<map2alm(x), b> = w <x, alm2map(b')> with b'_l0 = Re b_l0, b'_lm = b_lm / 2: the left side is good to 1e-10 max|x| sum|b|,
    the right side carries the float32 store of the map, 2^-24 max|map| w sum|x|; twice that is asserted."""
    lmax, N, F = 4 * nside - 1, 2, 3
    x = torch.from_numpy(fresh(sr.base_maps(nside)[:N, :, :F])).cuda()
    b = torch.from_numpy(fresh(sr.base_alm(lmax)[:N, :, :F])).cuda()
    a = sht.map2alm(x, nside, lmax=lmax)
    lhs = float((a.real * b.real + a.imag * b.imag).sum())
    bp = b.clone()
    bp[:, :lmax + 1] = b[:, :lmax + 1].real.to(b.dtype)
    bp[:, lmax + 1:] *= 0.5
    y = sht.alm2map(bp, nside)
    w = 4.0 * np.pi / (12 * nside * nside)
    rhs = w * float((x.double() * y.double()).sum())
    bound = 2 * (TOL_A * float(x.abs().max()) * float(b.abs().sum()) + 2.0 ** -24 * float(y.abs().max()) * w * float(x.abs().sum()))
    print(f"nside {nside}: {lhs:.12e} {rhs:.12e} bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound
    # the same through autograd: the gradient of <map2alm(x), b> is w alm2map(b')
    xg = x.clone().requires_grad_(True)
    a = sht.map2alm(xg, nside, lmax=lmax)
    (a.real * b.real + a.imag * b.imag).sum().backward()
    assert float((xg.grad.double() - w * y.double()).abs().max()) <= 2.0 ** -22 * w * float(y.abs().max())


@pytest.mark.parametrize("cap", (False, True))
def test_last_layer_of_a_network(cap):
    nside = 8
    ind = sr.footprints(nside)["cap"] if cap else None
    net = HealpyGCNN(nside, ind, [HealpyChebyshev(3, 4), HealpyPowerSpectrum(nside, indices=ind)])
    assert isinstance(net[1], HealpyPowerSpectrum)
    M = 12 * nside * nside if ind is None else ind.size
    x = torch.randn((2, M, 3), generator=torch.Generator().manual_seed(3)).cuda()
    y = net(x)
    assert tuple(y.shape) == (2, 3 * nside, 4)
    with torch.no_grad():
        assert torch.equal(y, net[1](net[0](x)))
    y.sum().backward()
    k = net[0].kernel.grad
    assert k is not None and bool(torch.isfinite(k).all()) and float(k.abs().max()) > 0
