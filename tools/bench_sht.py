#!/usr/bin/env python3
"""Time the spherical harmonic transforms of full-sky maps and HealpyPowerSpectrum on one GPU.

    python tools/bench_sht.py [--nsides 256,512,1024] [--shapes 8x1,4x4,2x16] [--reps 3] [--warmup 1] [--contender-nside 256]
                              [--host-nside 256] [--host-only]

Per nside (lmax = 3 nside - 1) and shape N x F (maps x channels):
(analysis)     _native.sht_analysis: map -> alm, the two kernels behind sht.map2alm(iter=0);
(synthesis)    _native.sht_synthesis: alm -> map, behind sht.alm2map;
(the stages)   the four entry points on their own, on one scratch array for the whole batch: which stage dominates;
(spectrum)     HealpyPowerSpectrum forward, and forward + backward (the backward is one synthesis);
(torch)        the contender, where its tables fit (--contender-nside and below: 2.4 GB of float64 lambda matrices at nside 256):
               the map reordered to RING by index_select, torch.fft.fft per ring length with the rings' phase factors and the
               fold of m onto the ring's length precomputed, then torch.matmul with the lambda matrix of every m -- tables from
               the host reference, built beforehand and not in the time;
(host)         healpix.map2alm(iter=0) in numpy at --host-nside, seconds per map (long-double recurrence; no GPU involved).

All device routes run in this process, alternating, after a warm-up.  A RUN times --reps back-to-back calls of a route between two
device events; three runs per route, interleaved route by route; the figure is the median run with the smallest and largest beside
it.  The contender's alm are compared with the kernels' (1e-9 max|x|) before anything is timed.  Scratch: the float64 F_m array,
16 (lmax + 1)(4 nside - 1) bytes per map and channel, at most _native.SHT_CHUNK_BYTES at a time in the compositions (but one whole
map).  Prints the figures and one JSON line.  The device routes need a GPU: there is no CPU fallback for them."""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "deepsphere-cosmo-tf2_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from deepsphere import _native, healpix  # noqa: E402
from deepsphere.healpy_layers import HealpyPowerSpectrum  # noqa: E402

RUNS = 3


def timed(fn, reps):
    """ms per call of `reps` back-to-back calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


class TorchContender:
    """map -> alm in plain torch on precomputed float64 tables (see the module text)."""

    def __init__(self, nside, lmax, dev):
        self.nside, self.lmax = nside, lmax
        nr, kshift, first = healpix._ring_phase0(nside)
        self.order = torch.as_tensor(healpix.ring2nest(nside, np.arange(12 * nside * nside, dtype=np.int64)), device=dev)
        m = np.arange(lmax + 1, dtype=np.int64)
        self.groups = []  # (first RING index, rings in the group, ring length, fold index [lmax + 1], phases [rings, lmax + 1])
        r = 0
        while r < 4 * nside - 1:
            r1 = r
            while r1 + 1 < 4 * nside - 1 and nr[r1 + 1] == nr[r]:
                r1 += 1
            n4 = 4 * int(nr[r])
            k0 = (m[None, :] * (1 - kshift[r:r1 + 1, None])) % (2 * n4)
            phase = torch.as_tensor(np.exp(-2j * np.pi * (k0 / (2.0 * n4))), device=dev)
            self.groups.append((int(first[r]), r1 + 1 - r, n4, torch.as_tensor(m % n4, device=dev), phase))
            r = r1 + 1
        w = 4.0 * np.pi / (12 * nside * nside)
        self.lam = [torch.as_tensor(w * healpix.legendre_lambda(nside, mm, lmax), device=dev) for mm in range(lmax + 1)]
        self.table_bytes = sum(t.numel() * 8 for t in self.lam) + sum(g[4].numel() * 16 for g in self.groups)

    def __call__(self, x):
        N, M, F = x.shape
        xr = x.index_select(1, self.order).to(torch.float64)
        fm = torch.empty((self.lmax + 1, 4 * self.nside - 1, N, F), dtype=torch.complex128, device=x.device)
        r = 0
        for first, rings, n4, fold, phase in self.groups:
            f = torch.fft.fft(xr[:, first:first + rings * n4].reshape(N, rings, n4, F), dim=2)
            fm[:, r:r + rings] = (f.index_select(2, fold) * phase[None, :, :, None]).permute(2, 1, 0, 3)
            r += rings
        fm = fm.reshape(self.lmax + 1, 4 * self.nside - 1, N * F)
        fr = torch.view_as_real(fm).reshape(self.lmax + 1, 4 * self.nside - 1, 2 * N * F)  # a real matrix product serves re and im
        alm = torch.cat([torch.matmul(self.lam[m], fr[m]) for m in range(self.lmax + 1)], dim=0)
        return torch.view_as_complex(alm.reshape(-1, N, F, 2)).permute(1, 0, 2)


def bench_shape(nside, N, F, reps, warmup, contender, dev, gen):
    lmax, M = 3 * nside - 1, 12 * nside * nside
    x = torch.randn((N, M, F), generator=gen, device=dev)
    alm = _native.sht_analysis(x, nside, lmax)
    y = torch.empty_like(x)
    fm = torch.empty(_native.sht_fm_shape(nside, lmax, N, F), dtype=torch.float64, device=dev)
    alm2 = torch.empty_like(alm)
    layer = HealpyPowerSpectrum(nside)
    xg = x.clone().requires_grad_(True)
    gcl = torch.randn((N, lmax + 1, F), generator=gen, device=dev)

    def fwd_bwd():
        xg.grad = None
        layer(xg).backward(gcl)

    cases = {
        "analysis": lambda: _native.sht_analysis(x, nside, lmax, out=alm2),
        "synthesis": lambda: _native.sht_synthesis(alm, nside, out=y),
        "ring_analysis": lambda: _native.sht_ring_analysis(x, nside, lmax, out=fm),
        "legendre_analysis": lambda: _native.sht_legendre_analysis(fm, nside, lmax, N, F, out=alm2),
        "legendre_synthesis": lambda: _native.sht_legendre_synthesis(alm, nside, out=fm),
        "ring_synthesis": lambda: _native.sht_ring_synthesis(fm, nside, lmax, N, F, out=y),
        "spectrum_fwd": lambda: layer(x),
        "spectrum_fwd_bwd": fwd_bwd,
    }
    if contender is not None:
        ref = contender(x)
        err = float((ref - alm).abs().max())
        if not err <= 1e-9 * float(x.abs().max()):
            raise SystemExit(f"nside {nside} N {N} F {F}: the torch contender differs from the kernels by {err:.3e}")
        cases["torch_analysis"] = lambda: contender(x)
    for _ in range(warmup):
        for fn in cases.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in cases}
    for _ in range(RUNS):  # alternating: drift of the machine hits every route alike
        for name, fn in cases.items():
            times[name].append(timed(fn, reps))
    ms = {name: statistics.median(t) for name, t in times.items()}
    step = _native.sht_chunk_maps(nside, lmax, F)
    scratch = 16 * (lmax + 1) * (4 * nside - 1) * F * min(step, N)
    print(f"nside {nside}, lmax {lmax}, N {N}, F {F}: F_m scratch {scratch / 1e6:.0f} MB a trip of {min(step, N)} map(s), "
          f"{fm.numel() * 8 / 1e6:.0f} MB for the whole batch")
    for name in cases:
        print(f"  {name:19s} {ms[name]:10.3f} ms  (min {min(times[name]):.3f}, max {max(times[name]):.3f}; {RUNS} runs of {reps} calls)", flush=True)
    ra, la = ms["ring_analysis"], ms["legendre_analysis"]
    print(f"  analysis: the {'ring' if ra > la else 'Legendre'} stage dominates ({ra:.3f} against {la:.3f} ms); synthesis: the "
          f"{'ring' if ms['ring_synthesis'] > ms['legendre_synthesis'] else 'Legendre'} stage "
          f"({ms['ring_synthesis']:.3f} against {ms['legendre_synthesis']:.3f} ms)")
    return {"nside": nside, "lmax": lmax, "N": N, "F": F, "ms": ms, "min_ms": {n: min(t) for n, t in times.items()},
            "max_ms": {n: max(t) for n, t in times.items()}, "scratch_bytes": scratch}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nsides", default="256,512,1024")
    ap.add_argument("--shapes", default="8x1,4x4,2x16", help="N x F, comma separated")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--contender-nside", type=int, default=256, help="the torch contender runs at this nside and below (0: never)")
    ap.add_argument("--host-nside", type=int, default=256, help="the host reference is timed at this nside (0: not at all)")
    ap.add_argument("--host-only", action="store_true", help="time the host reference only (no GPU needed)")
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    results, host = [], None
    if not args.host_only:
        _native.require_gpu()
        dev = torch.device("cuda", 0)
        gen = torch.Generator(device=dev).manual_seed(0)
        for nside in (int(v) for v in args.nsides.split(",")):
            contender = None
            if nside <= args.contender_nside:
                t0 = time.perf_counter()
                contender = TorchContender(nside, 3 * nside - 1, dev)
                print(f"nside {nside}: the torch contender's tables, {contender.table_bytes / 1e9:.2f} GB, built on the host in "
                      f"{time.perf_counter() - t0:.1f} s", flush=True)
            for N, F in shapes:
                results.append(bench_shape(nside, N, F, args.reps, args.warmup, contender, dev, gen))
            del contender
            torch.cuda.empty_cache()
    if args.host_nside:
        hn = args.host_nside
        xh = np.random.default_rng(0).standard_normal(12 * hn * hn)
        t0 = time.perf_counter()
        healpix.map2alm(xh, iter=0)
        host = {"nside": hn, "seconds_per_map": time.perf_counter() - t0}
        print(f"host reference, nside {hn}, lmax {3 * hn - 1}: healpix.map2alm(iter=0) {host['seconds_per_map']:.1f} s a map")
    print(json.dumps({"runs": RUNS, "reps": args.reps, "results": results, "host": host}))


if __name__ == "__main__":
    main()
