"""CPU tests of the harmonic-transform half of ``healpix.py`` (``alm_size``, ``alm_index``, ``legendre_lambda``, ``map2alm``,
``alm2map``, ``alm2cl``, ``anafast``, ``almxfl``), of ``deepsphere.sht`` and ``HealpyPowerSpectrum`` on CPU tensors and of the refusals
of the four ``dsph_sht_*`` entry points.  They make the numpy transform the proven reference of the GPU tests
(tests/test_gpu_sht.py), independently of any kernel: scipy's spherical harmonics, closed forms, the transpose identity, the
symmetry of the grid and the convergence of healpy's Jacobi iteration."""

import ctypes

import numpy as np
import pytest
import torch
from scipy.special import sph_harm_y

import deepsphere
import sht_ref as sr
from deepsphere import _native, healpix, healpy_layers, sht
from deepsphere.healpy_layers import HealpyPowerSpectrum


def test_alm_index_against_a_double_loop():
    for lmax in (0, 1, 2, 7, 31):
        i = 0
        for m in range(lmax + 1):
            for l in range(m, lmax + 1):
                assert healpix.alm_index(lmax, l, m) == i
                i += 1
        assert healpix.alm_size(lmax) == i
    ls, ms = np.array([3, 5, 5]), np.array([0, 2, 5])
    assert np.array_equal(healpix.alm_index(5, ls, ms), [3, 14, 20])
    with pytest.raises(ValueError):
        healpix.alm_size(-1)


@pytest.mark.parametrize("nside", (1, 2, 4, 8, 16))
def test_a_constant_map_has_a_00_only(nside):
    """a_00 = sqrt(4 pi) c.  The grid is invariant under phi -> phi + pi / 2 and under the reflection through the equator, so the
    coefficients with m not a multiple of 4 and those with l odd vanish by symmetry (to 1e-12); the others only as fast as the
    quadrature converges, so nothing is asserted of them."""
    c = 2.5
    lmax = 3 * nside - 1
    a = healpix.map2alm(np.full(12 * nside * nside, c), iter=0)
    assert a.shape == (healpix.alm_size(lmax),) and a.dtype == np.complex128
    assert abs(a[0] - np.sqrt(4 * np.pi) * c) <= 1e-12 * c
    for m in range(lmax + 1):
        for l in range(m, lmax + 1):
            if (l, m) != (0, 0) and (l % 2 == 1 or m % 4 != 0):
                assert abs(a[healpix.alm_index(lmax, l, m)]) <= 1e-12 * c, (l, m)


def test_lambda_against_scipy():
    nside, lmax = 8, 31
    theta = healpix._ring_info(nside, np.arange(1, 4 * nside))[3]
    for m in range(lmax + 1):
        lam = healpix.legendre_lambda(nside, m, lmax)
        assert lam.shape == (lmax + 1 - m, 4 * nside - 1) and lam.dtype == np.float64
        for l in range(m, lmax + 1):
            ref = sph_harm_y(l, m, theta, 0.0)
            assert np.abs(ref.imag).max() == 0 and np.abs(lam[l - m] - ref.real).max() <= 1e-12, (l, m)


@pytest.mark.parametrize("nside", (1, 4, 8))
def test_closed_forms(nside):
    """Y_10, Y_11 and Y_22 synthesised and compared pixel by pixel (a map is Re of a_l0 Y_l0, 2 Re of a_lm Y_lm)."""
    lmax = 2
    theta, phi = healpix.pix2ang(nside, np.arange(12 * nside * nside))
    forms = {(1, 0): np.sqrt(3 / (4 * np.pi)) * np.cos(theta),
             (1, 1): -np.sqrt(3 / (8 * np.pi)) * np.sin(theta) * np.exp(1j * phi),
             (2, 2): 0.25 * np.sqrt(15 / (2 * np.pi)) * np.sin(theta) ** 2 * np.exp(2j * phi)}
    for (l, m), y in forms.items():
        for coef in (1.0, 1j, 0.3 - 0.7j):
            alm = np.zeros(healpix.alm_size(lmax), dtype=np.complex128)
            alm[healpix.alm_index(lmax, l, m)] = coef
            ref = 2.0 * (coef * y).real if m else complex(coef).real * y
            assert np.abs(healpix.alm2map(alm, nside) - ref).max() <= 1e-13, (l, m, coef)
    alm = np.zeros(healpix.alm_size(lmax), dtype=np.complex128)
    alm[healpix.alm_index(lmax, 1, 1)] = 1.0
    assert np.array_equal(healpix.alm2map(alm, nside, nest=False), healpix.reorder(healpix.alm2map(alm, nside), n2r=True))


@pytest.mark.parametrize("nside", (4, 8))
def test_synthesis_and_analysis_are_transposes(nside):
    """<map2alm(x, iter=0), b> = w <x, alm2map(b')>, b'_l0 = Re b_l0, b'_lm = b_lm / 2, for every lmax of the grid."""
    rng = np.random.default_rng(nside)
    w = 4 * np.pi / (12 * nside * nside)
    for lmax in sr.lmaxes(nside):
        x = rng.standard_normal((12 * nside * nside, 2))
        n = healpix.alm_size(lmax)
        b = rng.standard_normal((n, 2)) + 1j * rng.standard_normal((n, 2))
        a = healpix.map2alm(x, lmax=lmax, iter=0)
        lhs = (a.real * b.real + a.imag * b.imag).sum()
        bp = b.copy()
        bp[:lmax + 1] = b[:lmax + 1].real
        bp[lmax + 1:] *= 0.5
        rhs = w * (x * healpix.alm2map(bp, nside)).sum()
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), np.abs(a).max() * np.abs(b).max()), (lmax, lhs, rhs)


@pytest.mark.parametrize("nside", (8, 16))
def test_jacobi_iterations_converge_on_a_band_limited_map(nside):
    lmax = nside
    rng = np.random.default_rng(nside)
    a0 = rng.standard_normal(healpix.alm_size(lmax)) + 1j * rng.standard_normal(healpix.alm_size(lmax))
    a0[:lmax + 1] = a0[:lmax + 1].real
    x = healpix.alm2map(a0, nside)
    errs = [np.abs(healpix.map2alm(x, lmax=lmax, iter=it) - a0).max() for it in (0, 1, 3)]
    print(errs)
    assert errs[0] > errs[1] > errs[2]
    assert healpix.map2alm(x).shape == (healpix.alm_size(3 * nside - 1),)  # healpy's default lmax


def test_orderings_shapes_and_argument_checks():
    nside = 4
    x = np.random.default_rng(0).standard_normal((192, 3))
    a = healpix.map2alm(x, iter=0)
    assert a.shape == (healpix.alm_size(11), 3)
    assert np.abs(healpix.map2alm(x[:, 1], iter=0) - a[:, 1]).max() <= 1e-14  # (the matrix products differ in shape)
    assert np.abs(healpix.map2alm(healpix.reorder(x, n2r=True), iter=0, nest=False) - a).max() <= 1e-14
    with pytest.raises(ValueError, match="lmax"):
        healpix.map2alm(x, lmax=16)
    with pytest.raises(ValueError):
        healpix.map2alm(x[:-1])
    with pytest.raises(ValueError, match="coefficients"):
        healpix.alm2map(np.zeros(5, dtype=complex), nside)
    for fn in (healpix.map2alm, healpix.alm2map, healpix.anafast):
        assert "NOT healpy's" in fn.__doc__


def test_alm2cl_anafast_and_almxfl_follow_the_definitions():
    lmax = 6
    rng = np.random.default_rng(1)
    a = rng.standard_normal((healpix.alm_size(lmax), 2)) + 1j * rng.standard_normal((healpix.alm_size(lmax), 2))
    cl = healpix.alm2cl(a)
    fl = rng.standard_normal(lmax + 1)
    scaled = healpix.almxfl(a, fl)
    for l in range(lmax + 1):
        s = np.abs(a[healpix.alm_index(lmax, l, 0)]) ** 2
        for m in range(1, l + 1):
            s = s + 2 * np.abs(a[healpix.alm_index(lmax, l, m)]) ** 2
            assert np.array_equal(scaled[healpix.alm_index(lmax, l, m)], a[healpix.alm_index(lmax, l, m)] * fl[l])
        assert np.abs(cl[l] - s / (2 * l + 1)).max() <= 1e-14 * s.max()
    assert healpix.alm2cl(a[:, 0]).shape == (lmax + 1,) and np.array_equal(healpix.alm2cl(a[:, 0]), cl[:, 0])
    assert np.all(healpix.almxfl(a, fl[:3])[healpix.alm_index(lmax, 3, 0):healpix.alm_index(lmax, 6, 0) + 1] == 0)
    x = rng.standard_normal(192)
    for it in (0, 1):
        assert np.array_equal(healpix.anafast(x, lmax=7, iter=it), healpix.alm2cl(healpix.map2alm(x, lmax=7, iter=it)))


def test_lambda_survives_the_exponent_range():
    """nside 1024, m = 1500, l up to 3071: sin^1500 theta of the first ring is 1e-4650, far below float64 and within the long
    double's range.  The discrete norm of lambda_lm e^{i m phi} over the pixels, sum_rings 4 nr w lambda^2 2 pi / (2 pi), is 1 up to
    the quadrature error."""
    nside, m, lmax = 1024, 1500, 3071
    lam = healpix.legendre_lambda(nside, m, lmax, dtype=np.longdouble)
    assert lam.shape == (lmax + 1 - m, 4 * nside - 1) and np.isfinite(lam).all()
    last = lam[-1]
    assert np.all(np.delete(last, 2 * nside - 1) != 0)  # (l + m is odd: the equator's value is the zero of symmetry)
    nr = healpix._ring_info(nside, np.arange(1, 4 * nside))[0]
    norm = float((4 * nr * (4 * np.pi / (12 * nside * nside)) * last ** 2).sum())
    print(norm)
    assert abs(norm - 1.0) <= 1e-5


def test_exports_and_signatures():
    for name in ("alm_size", "alm_index", "legendre_lambda", "map2alm", "alm2map", "alm2cl", "anafast", "almxfl"):
        assert name in healpix.__all__ and callable(getattr(healpix, name))
    assert deepsphere.HealpyPowerSpectrum is HealpyPowerSpectrum and "HealpyPowerSpectrum" in healpy_layers.__all__
    assert deepsphere.sht is sht and set(sht.__all__) == {"map2alm", "alm2map", "alm2cl", "anafast", "Footprint"}
    lib = _native.lib()
    for name, nargs in (("dsph_sht_ring_analysis", 11), ("dsph_sht_legendre_analysis", 8), ("dsph_sht_legendre_synthesis", 8),
                        ("dsph_sht_ring_synthesis", 11)):
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == nargs and hasattr(lib, name)
    for name in ("sht_ring_analysis", "sht_legendre_analysis", "sht_legendre_synthesis", "sht_ring_synthesis", "sht_analysis",
                 "sht_synthesis"):
        assert "out" in getattr(_native, name).__code__.co_varnames


def test_c_entry_points_refuse_bad_arguments():
    lib = _native.lib()
    buf = (ctypes.c_double * 4096)()
    p = ctypes.addressof(buf)
    q = p + 16384
    B, U = -1, -3

    def refused(rc, code, *words):
        assert rc == code, (rc, _native.last_error())
        for wd in words:
            assert wd in _native.last_error(), _native.last_error()

    for name in ("dsph_sht_ring_analysis", "dsph_sht_ring_synthesis"):
        fn, who = getattr(lib, name), name[5:]
        refused(fn(None, q, 1, 1, 1, 2, None, None, 12, 0, None), B, who, "NULL")
        refused(fn(p, None, 1, 1, 1, 2, None, None, 12, 0, None), B, who, "NULL")
        refused(fn(p, q, 1, 3, 1, 2, None, None, 108, 0, None), B, "power of two")
        refused(fn(p, q, 1, 4096, 1, 2, None, None, 12 * 4096**2, 0, None), U, "2048")
        refused(fn(p, q, 1, 1, 1, 4, None, None, 12, 0, None), B, "mmax = 4", "4 nside - 1")
        refused(fn(p, q, 1, 1, 1, -1, None, None, 12, 0, None), B, "mmax = -1")
        refused(fn(p, q, 1, 1, 0, 2, None, None, 12, 0, None), B, "F = 0")
        refused(fn(p, q, -1, 1, 1, 2, None, None, 12, 0, None), B, "N = -1")
        refused(fn(p, q, 1, 1, 1, 2, p, None, 12, 0, None), B, "come together")
        refused(fn(p, q, 1, 1, 1, 2, None, None, 11, 0, None), B, "without indices")
        refused(fn(p, q, 1, 1, 1, 2, p, p, 13, 0, None), B, "M = 13")
    refused(lib.dsph_sht_ring_analysis(p, q + 4, 1, 1, 1, 2, None, None, 12, 0, None), B, "fm", "8-byte")
    refused(lib.dsph_sht_ring_synthesis(p + 4, q, 1, 1, 1, 2, None, None, 12, 0, None), B, "fm", "8-byte")
    refused(lib.dsph_sht_ring_analysis(p, p + 16, 1, 1, 1, 2, None, None, 12, 0, None), B, "overlap")
    refused(lib.dsph_sht_ring_synthesis(p, p + 16, 1, 1, 1, 2, None, None, 12, 0, None), B, "overlap")
    for name in ("dsph_sht_legendre_analysis", "dsph_sht_legendre_synthesis"):
        fn, who = getattr(lib, name), name[5:]
        refused(fn(None, q, 1, 1, 1, 2, 0, None), B, who, "NULL")
        refused(fn(p, None, 1, 1, 1, 2, 0, None), B, who, "NULL")
        refused(fn(p, q, 1, 6, 1, 2, 0, None), B, "power of two")
        refused(fn(p, q, 1, 4096, 1, 2, 0, None), U, "2048")
        refused(fn(p, q, 1, 2, 1, 8, 0, None), B, "lmax = 8")
        refused(fn(p, q, 1, 1, 0, 2, 0, None), B, "F = 0")
        refused(fn(p, q, -2, 1, 1, 2, 0, None), B, "N = -2")
        refused(fn(p + 4, q, 1, 1, 1, 2, 0, None), B, "8-byte")
        refused(fn(p, q + 4, 1, 1, 1, 2, 0, None), B, "8-byte")
        refused(fn(p, p + 16, 1, 1, 1, 2, 0, None), B, "overlap")


def test_bindings_refuse_before_they_touch_the_gpu():
    x = torch.zeros(1, 192, 2)
    nalm = healpix.alm_size(11)
    a = torch.zeros(1, nalm, 2, dtype=torch.complex128)
    fm = torch.zeros(_native.sht_fm_shape(4, 11, 1, 2), dtype=torch.float64)
    bad = [
        (_native.sht_analysis, dict(x=x, nside=3, lmax=2), "power of two"),
        (_native.sht_analysis, dict(x=x, nside=4096, lmax=2), "2048"),
        (_native.sht_analysis, dict(x=x, nside=4, lmax=16), "lmax = 16"),
        (_native.sht_analysis, dict(x=x.double(), nside=4, lmax=11), "float32"),
        (_native.sht_analysis, dict(x=x[:, :-1], nside=4, lmax=11), "191"),
        (_native.sht_analysis, dict(x=x, nside=4, lmax=11, indices=torch.arange(192)), "come together"),
        (_native.sht_analysis, dict(x=x, nside=4, lmax=11, out=torch.zeros(1, nalm, 2)), "out must be"),
        (_native.sht_analysis, dict(x=x, nside=4, lmax=11), "HIP tensor"),
        (_native.sht_ring_analysis, dict(x=x, nside=4, lmax=11), "HIP tensor"),
        (_native.sht_synthesis, dict(alm=a.to(torch.complex64), nside=4), "complex128"),
        (_native.sht_synthesis, dict(alm=a[:, :-1], nside=4), "coefficients"),
        (_native.sht_synthesis, dict(alm=a, nside=2), "lmax = 11"),
        (_native.sht_synthesis, dict(alm=a, nside=4, out=torch.zeros(1, 192, 3)), "out must be"),
        (_native.sht_synthesis, dict(alm=a, nside=4), "HIP tensor"),
        (_native.sht_legendre_synthesis, dict(alm=a, nside=4), "HIP tensor"),
        (_native.sht_legendre_analysis, dict(fm=fm[:-1], nside=4, lmax=11, N=1, F=2), "fm must be"),
        (_native.sht_legendre_analysis, dict(fm=fm, nside=4, lmax=11, N=1, F=2), "HIP tensor"),
        (_native.sht_ring_synthesis, dict(fm=fm, nside=4, lmax=11, N=2, F=1, out=torch.zeros(1, 192, 2)), "out must be"),
        (_native.sht_ring_synthesis, dict(fm=fm, nside=4, lmax=11, N=1, F=2), "HIP tensor"),
    ]
    for fn, kwargs, match in bad:
        with pytest.raises(ValueError, match=match):
            fn(**kwargs)
    # 201 MB a column at nside 1024: 10 columns fit 2 GiB, 8 fill a block; a map of 16 channels is taken alone
    assert _native.sht_chunk_maps(1024, 3071, 1) == 8 and _native.sht_chunk_maps(1024, 3071, 4) == 2 and _native.sht_chunk_maps(1024, 3071, 16) == 1
    assert _native.sht_chunk_maps(1, 3, 17) == 960 and 960 * 17 <= _native.SHT_CHUNK_COLS and _native.sht_chunk_maps(1, 3, 1) == _native.SHT_CHUNK_COLS


def test_sht_and_the_layer_on_cpu_tensors():
    nside, N, F = 4, 2, 3
    lmax = 3 * nside - 1
    x = torch.randn(N, 192, F, generator=torch.Generator().manual_seed(0))
    a = sht.map2alm(x, nside)
    assert a.dtype == torch.complex128 and tuple(a.shape) == (N, healpix.alm_size(lmax), F)
    for n in range(N):
        assert np.abs(a[n].numpy() - healpix.map2alm(x[n].double().numpy(), iter=0)).max() <= 1e-13
    assert np.abs(sht.map2alm(x, nside, lmax=5, iter=2)[1].numpy() - healpix.map2alm(x[1].double().numpy(), lmax=5, iter=2)).max() <= 1e-13
    y = sht.alm2map(a, nside)
    assert y.dtype == torch.float32 and np.abs(y[1].numpy() - healpix.alm2map(a[1].numpy(), nside)).max() <= 2.0 ** -23 * float(y.abs().max())
    cl = sht.alm2cl(a)
    assert cl.dtype == torch.float64 and np.abs(cl[0].numpy() - healpix.alm2cl(a[0].numpy())).max() <= 1e-14 * float(cl.max())
    assert torch.equal(sht.anafast(x, nside), cl)
    # a footprint: the pseudo-spectrum of the zero-filled map
    ind = sr.footprints(nside)["cap"]
    layer = HealpyPowerSpectrum(nside, indices=ind, lmax=7, iter=1)
    assert not hasattr(layer, "p") and not hasattr(layer, "Fout") and layer.call == layer.forward
    full = np.zeros((192, F))
    full[ind] = x[0, ind].double().numpy()
    out = layer(x[:, ind].double())
    assert out.dtype == torch.float64 and tuple(out.shape) == (N, 8, F)
    assert np.abs(out[0].numpy() - healpix.anafast(full, lmax=7, iter=1)).max() <= 1e-12 * float(out.max())
    assert HealpyPowerSpectrum(nside)(x).dtype == torch.float32
    # alm2cl is differentiable where it runs in torch: the gradient of sum gC C_l is 2 mult gC_l a_lm / (2 l + 1)
    ag = a.clone().requires_grad_(True)
    gc = torch.randn(N, lmax + 1, F, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    (sht.alm2cl(ag) * gc).sum().backward()
    ls = np.concatenate([np.arange(m, lmax + 1) for m in range(lmax + 1)])
    mult = np.where(np.arange(ls.size) <= lmax, 1.0, 2.0)
    ref = 2 * (mult / (2 * ls + 1))[None, :, None] * gc.numpy()[:, ls] * a.numpy()
    assert np.abs(ag.grad.numpy() - ref).max() <= 1e-14 * np.abs(ref).max()
    with pytest.raises(ValueError, match="power of two"):
        HealpyPowerSpectrum(12)
    with pytest.raises(ValueError, match="2048"):
        HealpyPowerSpectrum(4096)
    with pytest.raises(ValueError, match="lmax"):
        HealpyPowerSpectrum(4, lmax=16)
    with pytest.raises(ValueError, match=r"191"):
        HealpyPowerSpectrum(4)(x[:, :-1])
