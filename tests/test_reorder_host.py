"""CPU tests of the RING <-> NEST index maths (``healpix.nest2ring`` / ``ring2nest`` / ``reorder`` / ``reorder_table`` /
``extend_indices(nest=False)``), of ``HealpyReorder`` on CPU tensors and of the refusals of ``_native.healpix_reorder`` and of the C
entry point, which all come before any launch.  Everything is bit for bit: a reorder moves values and computes none."""

import numpy as np
import pytest
import torch

from deepsphere import _native, healpix
from deepsphere.healpy_layers import HealpyReorder

NSIDES = (1, 2, 4, 8, 32, 64)


@pytest.fixture(scope="module")
def tables():
    """nside -> (nest2ring(arange), ring2nest(arange)), computed once."""
    out = {}
    for nside in NSIDES:
        ids = np.arange(12 * nside * nside, dtype=np.int64)
        out[nside] = (healpix.nest2ring(nside, ids), healpix.ring2nest(nside, ids))
    return out


@pytest.mark.parametrize("nside", NSIDES)
def test_permutation_and_inverse(tables, nside):
    n2r, r2n = tables[nside]
    ids = np.arange(12 * nside * nside, dtype=np.int64)
    assert n2r.dtype == np.int64 and r2n.dtype == np.int64
    assert np.array_equal(np.sort(n2r), ids)
    assert np.array_equal(n2r[r2n], ids) and np.array_equal(r2n[n2r], ids)


@pytest.mark.parametrize("nside", NSIDES)
def test_defining_order_of_ring(tables, nside):
    """RING lists the pixel centres by non-increasing z and, within a ring (equal z to 1e-12), by strictly increasing phi."""
    v = healpix.pix2vec(nside, tables[nside][1])
    z = v[:, 2]
    phi = np.mod(np.arctan2(v[:, 1], v[:, 0]), 2 * np.pi)
    dz = np.diff(z)
    assert np.all(dz <= 1e-12)
    same = np.abs(dz) <= 1e-12
    assert np.all(np.diff(phi)[same] > 0)


@pytest.mark.parametrize("nside", NSIDES)
def test_ring_sizes(tables, nside):
    z = healpix.pix2vec(nside, tables[nside][1])[:, 2]
    starts = np.concatenate(([0], np.nonzero(np.abs(np.diff(z)) > 1e-12)[0] + 1, [z.size]))
    sizes = np.diff(starts)
    want = [4 * i for i in range(1, nside)] + [4 * nside] * (2 * nside + 1) + [4 * i for i in range(nside - 1, 0, -1)]
    assert sizes.tolist() == want


def test_published_values():
    assert healpix.ring2nest(2, np.arange(10)).tolist() == [3, 7, 11, 15, 2, 1, 6, 5, 10, 9]
    assert int(healpix.ring2nest(16, 1504)) == 1130


@pytest.mark.parametrize("nside", (1, 2, 8, 8192))
def test_closed_forms(nside):
    assert int(healpix.nest2ring(nside, nside * nside - 1)) == 0
    assert int(healpix.nest2ring(nside, 11 * nside * nside)) == 12 * nside * nside - 1


def test_round_trip_at_nside_8192():
    """The integer square root of the caps is exact past 2^24; no full table is built."""
    nside = 8192
    npix = 12 * nside * nside
    i = np.arange(1, nside, dtype=np.int64)
    first, last = 2 * i * (i - 1), 2 * i * (i + 1) - 1  # of the north-cap rings
    ncap = 2 * nside * (nside - 1)
    belt = ncap + np.linspace(0, 2 * nside, 64).astype(np.int64) * 4 * nside  # first pixels of 64 belt rings
    rnd = np.random.default_rng(8192).integers(0, npix, size=10**6)
    for r in (first, last, npix - 1 - first, npix - 1 - last, belt, belt + 4 * nside - 1, rnd):
        assert r.min() >= 0 and r.max() < npix
        nest = healpix.ring2nest(nside, r)
        assert nest.min() >= 0 and nest.max() < npix
        assert np.array_equal(healpix.nest2ring(nside, nest), r)


def test_nside_must_be_a_power_of_two():
    for fn in (healpix.nest2ring, healpix.ring2nest):
        with pytest.raises(ValueError):
            fn(3, 0)


def test_reorder_round_trip_and_refusals(tables):
    m = np.random.default_rng(0).standard_normal((768, 3))
    n2r, r2n = tables[8]
    nest = healpix.reorder(m, r2n=True)
    assert np.array_equal(nest, m[n2r])  # NEST row i is RING row nest2ring(i)
    assert np.array_equal(healpix.reorder(nest, n2r=True), m)
    nest_t = healpix.reorder(m.T, r2n=True, axis=1)
    assert np.array_equal(nest_t, nest.T)
    assert np.array_equal(healpix.reorder(nest_t, n2r=True, axis=1), m.T)
    with pytest.raises(ValueError):
        healpix.reorder(m, r2n=True, n2r=True)
    with pytest.raises(ValueError):
        healpix.reorder(m)
    with pytest.raises(ValueError):
        healpix.reorder(m[:767], r2n=True)


@pytest.fixture(scope="module")
def footprint():
    return healpix.extend_indices(healpix.cap_indices(8, fraction=0.3), 8, 2)


def test_reorder_table(tables, footprint):
    n2r, r2n = tables[8]
    perm, indices_ring = healpix.reorder_table(8, footprint, r2n=True)
    assert perm.dtype == np.int32 and indices_ring.dtype == np.int64
    assert np.array_equal(indices_ring, np.sort(n2r[footprint]))
    ring_map = np.random.default_rng(1).standard_normal((768, 2))
    nest_map = ring_map[n2r]
    assert np.array_equal(ring_map[indices_ring][perm], nest_map[footprint])
    inv, indices_ring2 = healpix.reorder_table(8, footprint, r2n=False)
    assert np.array_equal(indices_ring2, indices_ring)
    assert np.array_equal(perm[inv], np.arange(footprint.size)) and np.array_equal(inv[perm], np.arange(footprint.size))
    assert np.array_equal(nest_map[footprint][inv], ring_map[indices_ring])


def test_extend_indices_in_ring_order(tables):
    n2r, r2n = tables[8]
    ids = np.sort(n2r[healpix.cap_indices(8, fraction=0.3)])
    got = healpix.extend_indices(ids, 8, 2, nest=False)
    assert np.array_equal(got, np.sort(healpix.nest2ring(8, healpix.extend_indices(healpix.ring2nest(8, ids), 8, 2))))
    assert np.array_equal(healpix.extend_indices(got, 8, 2, nest=False), got)
    assert np.all(np.isin(ids, got))


def _layer_cases(footprint):
    full = np.arange(192, dtype=np.int64)
    return (("full", 4, None, healpix.nest2ring(4, full), healpix.ring2nest(4, full)),
            ("partial", 8, footprint) + tuple(healpix.reorder_table(8, footprint, r2n=d)[0].astype(np.int64) for d in (True, False)))


def test_healpy_reorder_on_cpu_tensors(footprint):
    for name, nside, indices, to_nest, to_ring in _layer_cases(footprint):
        M = to_nest.size
        x = torch.randn(2, M, 3, generator=torch.Generator().manual_seed(3))
        l_r2n, l_n2r = HealpyReorder(nside, indices, r2n=True), HealpyReorder(nside, indices, r2n=False)
        assert l_r2n.r2n and not l_n2r.r2n
        if indices is not None:
            assert np.array_equal(l_r2n.indices, indices)
            assert np.array_equal(l_r2n.indices_ring, np.sort(healpix.nest2ring(nside, indices)))
        y = l_r2n(x)
        assert np.array_equal(y.numpy(), x.numpy()[:, to_nest]), name
        assert np.array_equal(l_n2r(x).numpy(), x.numpy()[:, to_ring]), name
        assert torch.equal(l_n2r(y), x), name
        for layer, opposite in ((l_r2n, to_ring), (l_n2r, to_nest)):
            xg = x.clone().requires_grad_(True)
            g = torch.randn(2, M, 3, generator=torch.Generator().manual_seed(4))
            (layer(xg) * g).sum().backward()
            assert np.array_equal(xg.grad.numpy(), g.numpy()[:, opposite]), name
        with pytest.raises(ValueError, match=rf"{M - 1}.*{M}"):
            l_r2n(x[:, :-1])


def test_layer_is_exported():
    import deepsphere
    from deepsphere import healpy_layers

    assert deepsphere.HealpyReorder is HealpyReorder and "HealpyReorder" in healpy_layers.__all__
    for name in ("nest2ring", "ring2nest", "reorder", "reorder_table"):
        assert name in healpix.__all__


def test_native_reorder_refuses_before_the_library_is_needed(monkeypatch):
    def no_library():
        raise AssertionError("the library was asked for before the arguments were checked")

    monkeypatch.setattr(_native, "lib", no_library)
    monkeypatch.setattr(_native, "require_gpu", no_library)
    with pytest.raises(ValueError, match="8192"):
        _native.healpix_reorder(torch.zeros(1, 12, 1), 16384, True)
    with pytest.raises(ValueError, match="float32"):
        _native.healpix_reorder(torch.zeros(1, 12 * 16, 1, dtype=torch.float64), 4, True)
    with pytest.raises(ValueError, match="191"):
        _native.healpix_reorder(torch.zeros(1, 191, 1), 4, True)
    with pytest.raises(ValueError, match="contiguous"):
        _native.healpix_reorder(torch.zeros(1, 2, 192).transpose(1, 2), 4, True)
    with pytest.raises(ValueError, match="out"):
        _native.healpix_reorder(torch.zeros(1, 192, 2), 4, True, out=torch.zeros(1, 192, 1))


def test_c_entry_refuses_before_any_launch():
    """Through the C ABI without a device: dummy non-NULL pointers that are never read."""
    lib = _native.lib()
    p, q = 4096, 1 << 30  # non-NULL, 16-byte aligned, far apart
    U, B = -3, -1  # DSPH_E_UNSUPPORTED, DSPH_E_BADARG

    def refused(rc, code, *words):
        msg = _native.last_error()
        assert rc == code and all(w in msg for w in words), (rc, msg)

    refused(lib.dsph_healpix_reorder(None, q, 1, 4, 1, 1, 0, None), B, "healpix_reorder", "NULL")
    refused(lib.dsph_healpix_reorder(p, None, 1, 4, 1, 1, 0, None), B, "healpix_reorder", "NULL")
    refused(lib.dsph_healpix_reorder(p, q, 1, 0, 1, 1, 0, None), B, "healpix_reorder", "power of two")
    refused(lib.dsph_healpix_reorder(p, q, 1, 3, 1, 1, 0, None), B, "healpix_reorder", "power of two")
    refused(lib.dsph_healpix_reorder(p, q, 1, 16384, 1, 1, 0, None), U, "healpix_reorder", "8192")
    refused(lib.dsph_healpix_reorder(p, q, 1, 4, 0, 1, 0, None), B, "healpix_reorder", "F = 0")
    refused(lib.dsph_healpix_reorder(p, q, -1, 4, 1, 1, 0, None), B, "healpix_reorder", "N = -1")
    refused(lib.dsph_healpix_reorder(p, p + 16, 1, 4, 1, 0, 0, None), B, "healpix_reorder", "overlap")
    refused(lib.dsph_healpix_reorder(p, p, 1, 4, 1, 1, 0, None), B, "healpix_reorder", "overlap")
