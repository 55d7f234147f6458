#!/usr/bin/env python3
"""Writes the ELL of the maps tools/asan/cimage_driver.cpp runs on (the quad-strip cases of run_plan_builders.py: the full-sphere
grid, the sphere without its last pixels -- an incomplete last tile --, partial-sky caps padded to superpixels) into DIR as
NAME.ell: int64 rows, int64 width, int32 cols[rows][width], float32 vals[rows][width].  numpy / scipy only, no sanitizer."""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = types.ModuleType("deepsphere")  # the package without its __init__ (which imports the torch layers)
pkg.__path__ = [os.path.join(ROOT, "deepsphere-cosmo-tf2_amd", "deepsphere")]
sys.modules["deepsphere"] = pkg
from deepsphere import healpix, utils  # noqa: E402


def dump(path, L):
    Lt, _ = utils.prepare_L(L, scale=0.75)
    cols, vals = utils.csr_to_ell(Lt)
    with open(path, "wb") as f:
        np.asarray(cols.shape, np.int64).tofile(f)
        np.ascontiguousarray(cols, np.int32).tofile(f)
        np.ascontiguousarray(vals, np.float32).tofile(f)


def main(out):
    os.makedirs(out, exist_ok=True)
    dump(os.path.join(out, "grid64.ell"), healpix.healpix_laplacian(64, mode="grid"))
    M = 12 * 64 * 64
    for drop in (100, 200, 256 + 37):
        dump(os.path.join(out, f"grid64_drop{drop}.ell"), healpix.healpix_laplacian(64, indices=np.arange(M - drop), mode="grid"))
    for nside, sup in ((64, 8), (128, 8), (64, 2)):
        idx = healpix.extend_indices(healpix.cap_indices(nside, fraction=1.0 / 3.0), nside, sup)
        dump(os.path.join(out, f"cap{nside}_{sup}.ell"), healpix.healpix_laplacian(nside, indices=idx, mode="grid"))


if __name__ == "__main__":
    main(sys.argv[1])
