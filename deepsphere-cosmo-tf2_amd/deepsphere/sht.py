"""Spherical harmonic transforms and power spectra of HEALPix maps on torch tensors, under healpy's names.

``map2alm``, ``alm2map``, ``alm2cl`` and ``anafast`` take the layout of the layers here: maps are ``(N, M, F)`` float32 in NEST
order (``M`` the pixels of the full sky or of a footprint ``indices``), coefficients ``(N, nalm, F)`` complex128 in healpy's packed
layout (``healpix.alm_index``), spectra ``(N, lmax + 1, F)`` float64.  Equal pixel weights w = 4 pi / npix, i.e. healpy with
``use_weights=False``; ``iter`` defaults to 0 here (healpy: 3).

HIP tensors run the kernels of ``csrc/healpix_sht.hip`` (``_native.sht_analysis`` / ``sht_synthesis``: float64 arithmetic, float32
maps) and are differentiable: the two transforms are each other's adjoints up to the weight and the multiplicity of m > 0, so a
backward is one transform of the other kind.  CPU tensors run the numpy reference of ``healpix`` (``healpix.map2alm`` ...), without
autograd.  On a footprint the transforms are those of the zero-filled full-sky map (a pseudo-spectrum), read back at the footprint.
"""

import numpy as np
import torch

from . import _native, healpix

__all__ = ["map2alm", "alm2map", "alm2cl", "anafast", "Footprint"]

_CL = {}     # (lmax, device) -> (l of every packed index, its weight mult / (2 l + 1): mult = 1 for m = 0, else 2)


class Footprint:
    """The pixel set of partial-sky maps, checked once, with its device tables (indices int64, lut int32) kept per device: what a
    caller that transforms many batches on one set (``HealpyPowerSpectrum``) passes as ``indices``."""

    def __init__(self, nside, indices):
        self.nside = healpix._check_nside(nside)
        if isinstance(indices, torch.Tensor):
            indices = indices.detach().cpu().numpy()
        self.ind = healpix._index_set(self.nside, indices)  # None: the full sky
        self._dev = {}

    def on(self, device):
        """-> (indices, lut) on a HIP ``device``; (None, None) for the full sky or a CPU device."""
        if self.ind is None or device.type != "cuda":
            return None, None
        if str(device) not in self._dev:
            self._dev[str(device)] = healpix._device_lut(self.nside, self.ind, device)
        return self._dev[str(device)]


def _footprint(nside, indices, device):
    """-> (ind numpy or None, indices tensor or None, lut tensor or None) on ``device`` (tensors only for a HIP device)."""
    fp = indices if isinstance(indices, Footprint) else Footprint(nside, indices)
    if fp.nside != nside:
        raise ValueError(f"the footprint was built for nside {fp.nside}, the transform is asked for nside {nside}")
    return (fp.ind,) + tuple(fp.on(device))


def _pixel_weight(nside):
    return 4.0 * np.pi / healpix.nside2npix(nside)


def _m0_and_rest(lmax):
    return slice(0, lmax + 1), slice(lmax + 1, None)  # the packed layout is m-major: m = 0 comes first


class _Synthesis(torch.autograd.Function):
    """map_p = sum_l a_l0 Y_l0(p) + 2 Re sum_{m > 0} a_lm Y_lm(p).  For a gradient d on the map the gradient on alm is
    g_l0 = Re(analysis(d)_l0) / w and g_lm = 2 analysis(d)_lm / w."""

    @staticmethod
    def forward(ctx, alm, nside, ti, lut):
        ctx.args = (nside, ti, lut, int(alm.shape[1]))
        return _native.sht_synthesis(alm.contiguous(), nside, ti, lut)

    @staticmethod
    def backward(ctx, d):
        nside, ti, lut, nalm = ctx.args
        lmax = _native._sht_lmax_of("alm2map", nalm)
        a = _Analysis.apply(d.to(torch.float32), nside, lmax, ti, lut) / _pixel_weight(nside)
        m0, rest = _m0_and_rest(lmax)
        g = torch.empty_like(a)
        g[:, m0] = a[:, m0].real.to(a.dtype)
        g[:, rest] = 2.0 * a[:, rest]
        return g, None, None, None


class _Analysis(torch.autograd.Function):
    """alm = w sum_p Y*_lm(p) x_p.  For a gradient g on alm (torch's convention: d / d re + i d / d im) the input gradient is
    w synthesis(g') with g'_l0 = Re g_l0 and g'_lm = g_lm / 2 (m > 0), read at the footprint."""

    @staticmethod
    def forward(ctx, x, nside, lmax, ti, lut):
        ctx.args = (nside, lmax, ti, lut)
        return _native.sht_analysis(x.contiguous(), nside, lmax, ti, lut)

    @staticmethod
    def backward(ctx, g):
        nside, lmax, ti, lut = ctx.args
        m0, rest = _m0_and_rest(lmax)
        b = torch.empty_like(g, memory_format=torch.contiguous_format)
        w = _pixel_weight(nside)  # (applied to the float64 coefficients: the map is rounded to float32 once)
        b[:, m0] = (w * g[:, m0].real).to(g.dtype)
        b[:, rest] = (0.5 * w) * g[:, rest]
        return _Synthesis.apply(b, nside, ti, lut), None, None, None, None


def _check_maps(what, x, nside, ind):
    if not (isinstance(x, torch.Tensor) and x.dim() == 3 and x.is_floating_point()):
        raise ValueError(f"{what}: the maps must be a floating-point (N, M, F) tensor")
    M = healpix.nside2npix(nside) if ind is None else int(ind.size)
    if x.shape[1] != M or x.shape[2] < 1:
        raise ValueError(f"{what}: maps of shape {tuple(x.shape)} do not fit {M} pixels (nside {nside}) with at least one channel")


def map2alm(x, nside, lmax=None, iter=0, indices=None):  # noqa: A002  (healpy's argument name)
    """The harmonic coefficients of the NEST maps ``x`` (N, M, F): complex128 (N, nalm, F), mmax = lmax (default 3 nside - 1).
    ``iter = 0`` is the quadrature with equal weights; ``iter > 0`` adds healpy's Jacobi steps alm += map2alm(x - alm2map(alm)),
    composed of the two transforms (and differentiable through them).  ``indices``: the footprint of a partial-sky map, sorted
    NEST ids or a ``Footprint``."""
    nside = healpix._check_nside(nside)
    lmax = healpix._sht_lmax(nside, lmax)
    ind, ti, lut = _footprint(nside, indices, x.device if isinstance(x, torch.Tensor) else torch.device("cpu"))
    _check_maps("map2alm", x, nside, ind)
    if not x.is_cuda:
        full = _host_full(x, nside, ind)
        a = healpix.map2alm(full, lmax=lmax, iter=int(iter)) if full.shape[1] else np.zeros((healpix.alm_size(lmax), 0), dtype=np.complex128)
        return torch.from_numpy(np.ascontiguousarray(a.reshape(-1, x.shape[0], x.shape[2]).transpose(1, 0, 2)))
    if x.dtype != torch.float32:
        raise ValueError("map2alm: HIP maps must be float32")
    if int(iter) > 0 and ti is not None:
        # healpy iterates on the zero-filled map: the residual outside the footprint, minus the synthesised map there, counts
        x = x.new_zeros((x.shape[0], healpix.nside2npix(nside), x.shape[2])).index_copy(1, ti, x)
        ti = lut = None
    alm = _Analysis.apply(x, nside, lmax, ti, lut)
    for _ in range(int(iter)):
        alm = alm + _Analysis.apply(x - _Synthesis.apply(alm, nside, ti, lut), nside, lmax, ti, lut)
    return alm


def _host_full(x, nside, ind):
    """CPU maps (N, M, F) -> float64 [npix, N F] zero-filled full-sky maps."""
    v = x.detach().to(torch.float64).numpy().transpose(1, 0, 2).reshape(x.shape[1], -1)
    if ind is None:
        return v
    full = np.zeros((healpix.nside2npix(nside), v.shape[1]), dtype=np.float64)
    full[ind] = v
    return full


def alm2map(alm, nside, indices=None):
    """The NEST maps (N, M, F) float32 of the packed coefficients ``alm`` (N, nalm, F) complex128; on a footprint the full-sky
    map read at ``indices``.  The m = 0 terms count once (their imaginary parts are ignored), the m > 0 terms as 2 Re."""
    nside = healpix._check_nside(nside)
    if not (isinstance(alm, torch.Tensor) and alm.dim() == 3 and alm.dtype == torch.complex128):
        raise ValueError("alm2map: alm must be a complex128 (N, nalm, F) tensor")
    ind, ti, lut = _footprint(nside, indices, alm.device)
    if not alm.is_cuda:
        N, nalm, F = alm.shape
        a = alm.detach().numpy().transpose(1, 0, 2).reshape(nalm, -1)
        m = healpix.alm2map(a, nside) if a.shape[1] else np.zeros((healpix.nside2npix(nside), 0))
        m = m if ind is None else m[ind]
        return torch.from_numpy(np.ascontiguousarray(m.reshape(-1, N, F).transpose(1, 0, 2))).to(torch.float32)
    return _Synthesis.apply(alm, nside, ti, lut)


def _cl_tables(lmax, device):
    key = (int(lmax), str(device))
    if key not in _CL:
        if len(_CL) >= 16:
            _CL.clear()
        ls = np.concatenate([np.arange(m, lmax + 1) for m in range(lmax + 1)])
        mult = np.concatenate([np.full(lmax + 1 - m, 1.0 if m == 0 else 2.0) for m in range(lmax + 1)])
        _CL[key] = (torch.as_tensor(ls, device=device), torch.as_tensor(mult / (2.0 * ls + 1.0), device=device))
    return _CL[key]


class _Alm2Cl(torch.autograd.Function):
    """C_l = (|a_l0|^2 + 2 sum_{m > 0} |a_lm|^2) / (2 l + 1), summed over m in ascending order (no atomics); the gradient on a_lm
    is 2 mult gC_l a_lm / (2 l + 1), a gather."""

    M_BLOCK = 32

    @staticmethod
    def forward(ctx, alm):
        N, nalm, F = alm.shape
        lmax = _native._sht_lmax_of("alm2cl", nalm)
        ls, wt = _cl_tables(lmax, alm.device)
        ctx.save_for_backward(alm)
        p = (alm.real ** 2 + alm.imag ** 2) * wt[None, :, None]
        cl = torch.zeros((N, lmax + 1, F), dtype=torch.float64, device=alm.device)
        l = torch.arange(lmax + 1, device=alm.device)
        for m0 in range(0, lmax + 1, _Alm2Cl.M_BLOCK):
            m = torch.arange(m0, min(m0 + _Alm2Cl.M_BLOCK, lmax + 1), device=alm.device)
            idx = (m * (2 * lmax + 1 - m) // 2)[:, None] + l[None, :]
            ok = l[None, :] >= m[:, None]
            block = p[:, torch.where(ok, idx, torch.zeros_like(idx)).reshape(-1)].reshape(N, m.numel(), lmax + 1, F)
            cl += (block * ok[None, :, :, None]).sum(dim=1)
        return cl

    @staticmethod
    def backward(ctx, gcl):
        (alm,) = ctx.saved_tensors
        lmax = _native._sht_lmax_of("alm2cl", alm.shape[1])
        ls, wt = _cl_tables(lmax, alm.device)
        return (2.0 * gcl.to(torch.float64).index_select(1, ls) * wt[None, :, None]) * alm


def alm2cl(alm):
    """The auto power spectra (N, lmax + 1, F) float64 of packed coefficients (N, nalm, F), like ``hp.alm2cl`` per map and channel."""
    if not (isinstance(alm, torch.Tensor) and alm.dim() == 3 and alm.is_complex()):
        raise ValueError("alm2cl: alm must be a complex (N, nalm, F) tensor")
    return _Alm2Cl.apply(alm.to(torch.complex128))


def anafast(x, nside, lmax=None, iter=0, indices=None):  # noqa: A002
    """``alm2cl(map2alm(x, nside, lmax, iter, indices))``: the auto power spectrum of every map and channel, (N, lmax + 1, F) float64."""
    return alm2cl(map2alm(x, nside, lmax=lmax, iter=iter, indices=indices))
