"""Shared helpers of the harmonic-transform tests (tests/test_sht_host.py, tests/test_gpu_sht.py; not collected by pytest): seeded
maps and coefficients, footprints, the (nside, lmax) grid and the host references of the four stages, computed once per (nside,
lmax) for the widest batch and sliced by the cases (the transforms act column by column).  The references are
``deepsphere.healpix``'s numpy functions, proven on the CPU in tests/test_sht_host.py; what is cached is never written."""

import functools

import numpy as np
import torch

from deepsphere import healpix

NSIDES = (1, 2, 4, 8, 16, 32)
FS = (1, 3, 4, 17)
NS = (1, 3)
N_MAX, F_MAX = max(NS), max(FS)


def lmaxes(nside):
    """0, 1, 2 nside + 1, 3 nside - 1 and 4 nside - 1 (m above Nyquist on every cap ring; at nside 1 on all rings)."""
    return tuple(sorted({0, 1, 2 * nside + 1, 3 * nside - 1, 4 * nside - 1}))


GRID = tuple((ns, lm) for ns in NSIDES for lm in lmaxes(ns))


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def base_maps(nside, seed=0):
    """float32 maps (N_MAX, npix, F_MAX) as a read-only numpy array: the cases take [:N, :, :F]."""
    g = torch.Generator().manual_seed(7000 + 10 * nside + seed)
    return frozen(torch.randn((N_MAX, 12 * nside * nside, F_MAX), generator=g).numpy())


@functools.lru_cache(maxsize=None)
def base_alm(lmax, seed=0):
    """complex128 coefficients (N_MAX, nalm, F_MAX), the a_l0 with imaginary parts too (a synthesis ignores them)."""
    rng = np.random.default_rng(9000 + lmax + seed)
    shape = (N_MAX, healpix.alm_size(lmax), F_MAX)
    return frozen(rng.standard_normal(shape) + 1j * rng.standard_normal(shape))


def footprints(nside):
    npix = 12 * nside * nside
    return {"cap": np.sort(healpix.cap_indices(nside, fraction=1.0 / 3.0)), "pair": np.array([3, npix - 5], dtype=np.int64)}


def columns(a):
    """(N, rows, F) -> [rows, N F]: column c = n F + f."""
    return np.ascontiguousarray(np.transpose(a, (1, 0, 2)).reshape(a.shape[1], -1))


def uncolumns(a, N, F):
    """[rows, N F] -> (N, rows, F)."""
    return np.ascontiguousarray(np.transpose(a.reshape(a.shape[0], N, F), (1, 0, 2)))


def ring_order(nside):
    return healpix.ring2nest(nside, np.arange(12 * nside * nside, dtype=np.int64))  # ring_map = nest_map[ring_order]


def host_fm(x, nside, lmax):
    """F_m of NEST maps (N, npix, F) float64: complex128 [lmax + 1, 4 nside - 1, N F]."""
    return healpix._ring_transform(columns(np.asarray(x, dtype=np.float64))[ring_order(nside)], nside, lmax)


def host_legendre_analysis(fm, nside, lmax):
    """[lmax + 1, rings, C] -> [nalm, C]."""
    w = 4.0 * np.pi / (12 * nside * nside)
    out = np.zeros((healpix.alm_size(lmax), fm.shape[2]), dtype=np.complex128)
    for m in range(lmax + 1):
        i0 = int(healpix.alm_index(lmax, m, m))
        out[i0:i0 + lmax + 1 - m] = w * (healpix.legendre_lambda(nside, m, lmax) @ fm[m])
    return out


def host_legendre_synthesis(alm, nside, lmax):
    """[nalm, C] -> [lmax + 1, rings, C]."""
    out = np.zeros((lmax + 1, 4 * nside - 1, alm.shape[1]), dtype=np.complex128)
    for m in range(lmax + 1):
        i0 = int(healpix.alm_index(lmax, m, m))
        out[m] = healpix.legendre_lambda(nside, m, lmax).T @ alm[i0:i0 + lmax + 1 - m]
    return out


def host_ring_synthesis(fm, nside):
    """[lmax + 1, rings, C] -> NEST maps [npix, C] float64."""
    return healpix._ring_synthesis(fm, nside)[healpix.nest2ring(nside, np.arange(12 * nside * nside, dtype=np.int64))]


@functools.lru_cache(maxsize=None)
def analysis_reference(nside, lmax):
    """-> (fm [lmax + 1, rings, C], alm [nalm, C]) of base_maps(nside), C = N_MAX F_MAX."""
    fm = host_fm(base_maps(nside), nside, lmax)
    return frozen(fm), frozen(host_legendre_analysis(fm, nside, lmax))


@functools.lru_cache(maxsize=None)
def synthesis_reference(nside, lmax):
    """-> (fm, maps [npix, C] float64) of base_alm(lmax)."""
    fm = host_legendre_synthesis(columns(base_alm(lmax)), nside, lmax)
    return frozen(fm), frozen(host_ring_synthesis(fm, nside))


def pick(cols, N, F):
    """Columns of the first N maps and F channels out of a [..., N_MAX F_MAX] reference."""
    idx = (np.arange(N)[:, None] * F_MAX + np.arange(F)[None, :]).reshape(-1)
    return cols[..., idx]


def fm_to_tensor(fm, device="cpu"):
    """complex [lmax + 1, rings, C] -> float64 tensor [lmax + 1, rings, C, 2]."""
    return torch.view_as_real(torch.from_numpy(np.ascontiguousarray(fm))).contiguous().to(device)


def fm_to_numpy(t):
    return torch.view_as_complex(t.cpu().contiguous()).numpy()
