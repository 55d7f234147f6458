"""GPU tests of the RING <-> NEST kernel (``dsph_healpix_reorder``) and of ``HealpyReorder`` on it (``pytest -m gpu``).

The reference is the numpy table ``healpix.nest2ring(nside, arange)`` (proven on the CPU in tests/test_reorder_host.py): NEST row i of
a map is RING row ``nest2ring(i)``.  A reorder moves values and computes none, so every comparison is ``torch.equal``.  Outputs are
NaN-filled views between sentinel bands (``large_map_ref.Guarded``): a row that was not written fails as NaN, a write outside the map
fails the band check.

The kernel has two forms, rows under 32 floats through an LDS image of a block of pixels (block edge 64, 32, 16, 8 for F = 1, 2-4,
5-16, 17-31, at most nside) and wider rows copied row by row (blocks of 8 x 8), each with 1, 2 or 4 floats per access by F and the
alignment of the maps, and a grid of min(N, 65535) maps in y.
"""

import numpy as np
import pytest
import torch

import large_map_ref as lm
from deepsphere import _native, healpix
from deepsphere.healpy_layers import HealpyChebyshev, HealpyReorder
from deepsphere.healpy_networks import HealpyGCNN
from helpers import offset_view

pytestmark = pytest.mark.gpu

NSIDES = (1, 2, 4, 16, 32, 64, 128)
FS = (1, 2, 3, 4, 5, 8, 16, 17, 64)
_TABLES = {}


def n2r_table(nside):
    """nest2ring(arange) of ``nside`` as an int64 tensor on the device, computed once per process and never written."""
    if nside not in _TABLES:
        _TABLES[nside] = torch.as_tensor(healpix.nest2ring(nside, np.arange(12 * nside * nside, dtype=np.int64))).cuda()
    return _TABLES[nside]


def expected(x, nside, to_nest):
    t = n2r_table(nside)
    if to_nest:
        return x.index_select(1, t)
    out = torch.empty_like(x)
    out[:, t] = x  # RING row nest2ring(i) = NEST row i
    return out


def run_case(nside, F, N, to_nest, mis_x=0, mis_y=0, seed=0):
    M = 12 * nside * nside
    x = torch.randn((N, M, F), generator=torch.Generator().manual_seed(1000 * nside + 10 * F + seed))
    xd = offset_view(x, mis_x) if mis_x else x.cuda()
    before = lm.checksum(xd)
    g = lm.Guarded((N, M, F), device="cuda", misalign=mis_y)
    out = _native.healpix_reorder(xd, nside, to_nest, out=g.view)
    torch.cuda.synchronize()
    assert out.data_ptr() == g.view.data_ptr()
    g.check(f"nside {nside} F {F} N {N} to_nest {to_nest}")
    assert lm.checksum(xd) == before
    assert torch.equal(out, expected(xd, nside, to_nest)), (nside, F, N, to_nest)


CASES = sorted({(ns, F, 1) for ns in NSIDES for F in (1, 4, 17)} | {(ns, F, 1) for ns in (2, 32, 64) for F in FS}
               | {(32, 4, 3), (16, 3, 3), (32, 64, 3), (4, 33, 3)})


@pytest.mark.parametrize("to_nest", (True, False), ids=("r2n", "n2r"))
@pytest.mark.parametrize("nside,F,N", CASES)
def test_kernel_against_the_numpy_table(nside, F, N, to_nest):
    run_case(nside, F, N, to_nest)


@pytest.mark.parametrize("to_nest", (True, False), ids=("r2n", "n2r"))
@pytest.mark.parametrize("nside,F,mis_x,mis_y", [(32, 4, 1, 0), (32, 4, 0, 1), (64, 1, 3, 0), (64, 1, 0, 2), (32, 64, 1, 0), (32, 64, 0, 3),
                                                 (16, 2, 2, 2)])
def test_views_off_16_byte_alignment(nside, F, mis_x, mis_y, to_nest):
    """A view 4, 8 or 12 bytes off on either side takes narrower accesses (``(16, 2, 2, 2)``: both 8 bytes off, two floats each)."""
    run_case(nside, F, 2, to_nest, mis_x, mis_y)


@pytest.mark.parametrize("F", (1, 16))
def test_round_trip(F):
    x = torch.randn((2, 12 * 64 * 64, F), generator=torch.Generator().manual_seed(F)).cuda()
    assert torch.equal(_native.healpix_reorder(_native.healpix_reorder(x, 64, True), 64, False), x)
    assert torch.equal(_native.healpix_reorder(_native.healpix_reorder(x, 64, False), 64, True), x)


@pytest.mark.parametrize("F", (1, 32))
def test_maps_beyond_the_grid_take_a_second_trip(F):
    """N = 65,536 maps at nside 1: one more than the grid's y extent, in both forms."""
    run_case(1, F, 65536, True)
    run_case(1, F, 65536, False)


def test_refusals_on_the_device():
    x = torch.zeros((1, 192, 2), device="cuda")
    with pytest.raises(ValueError, match="overlap"):
        _native.healpix_reorder(x, 4, True, out=x)
    e = _native.healpix_reorder(torch.zeros((0, 192, 2), device="cuda"), 4, True)
    assert e.shape == (0, 192, 2)


@pytest.mark.parametrize("F", (1, 4, 64))
def test_healpy_reorder_full_sky(F):
    nside = 16
    x = torch.randn((2, 12 * nside * nside, F), generator=torch.Generator().manual_seed(5)).cuda()
    g = torch.randn((2, 12 * nside * nside, F), generator=torch.Generator().manual_seed(6)).cuda()
    for r2n in (True, False):
        layer = HealpyReorder(nside, r2n=r2n)
        xg = x.clone().requires_grad_(True)
        y = layer(xg)
        assert torch.equal(y.detach(), expected(x, nside, r2n))
        (y * g).sum().backward()
        assert torch.equal(xg.grad, expected(g, nside, not r2n))
    with pytest.raises(ValueError, match=r"3071.*3072"):
        HealpyReorder(nside)(x[:, :-1])


@pytest.fixture(scope="module")
def footprint():
    return healpix.extend_indices(healpix.cap_indices(16, fraction=0.3), 16, 4)


def test_healpy_reorder_partial_sky(footprint):
    x = torch.randn((3, footprint.size, 5), generator=torch.Generator().manual_seed(7))
    g = torch.randn((3, footprint.size, 5), generator=torch.Generator().manual_seed(8))
    for r2n in (True, False):
        layer = HealpyReorder(16, footprint, r2n=r2n)
        xc, xd = x.clone().requires_grad_(True), x.cuda().requires_grad_(True)
        yc, yd = layer(xc), layer(xd)
        assert yd.is_cuda and torch.equal(yd.detach().cpu(), yc.detach())
        (yc * g).sum().backward()
        (yd * g.cuda()).sum().backward()
        assert torch.equal(xd.grad.cpu(), xc.grad)
    # the RING side of the set against the full-sky kernel: a full RING map's rows indices_ring, reordered, are the NEST map's rows
    full = torch.randn((1, 12 * 16 * 16, 5), generator=torch.Generator().manual_seed(9)).cuda()
    layer = HealpyReorder(16, footprint, r2n=True)
    part = layer(full[:, torch.as_tensor(layer.indices_ring).cuda()])
    assert torch.equal(part, _native.healpix_reorder(full, 16, True)[:, torch.as_tensor(footprint).cuda()])


def test_inside_a_network(footprint):
    """RING in, RING out: [reorder, Chebyshev, reorder] on the RING map equals the one-layer network on the NEST map, reordered."""
    torch.manual_seed(11)
    ring_net = HealpyGCNN(16, footprint, [HealpyReorder(16, footprint, r2n=True), HealpyChebyshev(K=3, Fout=4),
                                          HealpyReorder(16, footprint, r2n=False)])
    nest_net = HealpyGCNN(16, footprint, [HealpyChebyshev(K=3, Fout=4)])
    assert isinstance(ring_net[0], HealpyReorder) and isinstance(ring_net[2], HealpyReorder)
    x_nest = torch.randn((2, footprint.size, 3), generator=torch.Generator().manual_seed(12)).cuda()
    to_ring = HealpyReorder(16, footprint, r2n=False)
    x_ring = to_ring(x_nest)
    with torch.no_grad():
        nest_net(x_nest)  # builds the weights
        ring_net(x_ring)
        for dst, src in zip(ring_net.parameters(), nest_net.parameters()):
            dst.copy_(src)
        y_ring, y_nest = ring_net(x_ring), nest_net(x_nest)
    assert len(list(ring_net.parameters())) == len(list(nest_net.parameters())) > 0
    assert y_ring.shape == (2, footprint.size, 4)
    assert torch.equal(y_ring, to_ring(y_nest))


def test_past_2_31_elements():
    """nside 8192, N 3, F 1: 2,415,919,104 elements (9.7 GB) per side, both directions.  Checks: the int64 sum of the bit patterns of
    every map before and after, windows of output rows against the pixelwise host conversion of those ids only (first and last 4,096
    rows, 4,096 rows either side of elements 2^29, 2^30 and 2^31, the cap / belt boundaries of every map, 2^20 random rows), the
    input's checksum, the guard bands, and the whole round trip against the input.  No full host table is built."""
    nside, N = 8192, 3
    npix = 12 * nside * nside
    ncap = 2 * nside * (nside - 1)
    x = torch.randn((N, npix, 1), device="cuda", generator=torch.Generator(device="cuda").manual_seed(31))
    sums_x = [lm.checksum(x[n]) for n in range(N)]
    W = 4096
    flat = [np.arange(W), np.arange(N * npix - W, N * npix)] + [np.arange((1 << p) - W, (1 << p) + W) for p in (29, 30, 31)]
    flat.append(np.random.default_rng(31).integers(0, N * npix, size=1 << 20))
    flat = np.unique(np.concatenate(flat).astype(np.int64))
    seams = np.concatenate([np.arange(c - W, c + W) for c in (ncap, npix - ncap)]).astype(np.int64)  # RING ids

    def check_rows(out, src, out_flat, to_nest):
        """out.flat[row] == src.flat[map * npix + convert(pixel)] for the output rows ``out_flat``."""
        n, p = out_flat // npix, out_flat % npix
        q = healpix.nest2ring(nside, p) if to_nest else healpix.ring2nest(nside, p)
        a = out.reshape(-1).index_select(0, torch.as_tensor(out_flat).cuda())
        b = src.reshape(-1).index_select(0, torch.as_tensor(n * npix + q).cuda())
        assert torch.equal(a, b)

    def seam_rows(to_nest):  # output rows whose RING id lies at a cap / belt boundary, in every map
        p = healpix.ring2nest(nside, seams) if to_nest else seams
        return np.concatenate([n * npix + p for n in range(N)])

    g1 = lm.Guarded((N, npix, 1), device="cuda")
    y1 = _native.healpix_reorder(x, nside, True, out=g1.view)
    torch.cuda.synchronize()
    g1.check("to_nest")
    assert [lm.checksum(x[n]) for n in range(N)] == sums_x
    assert [lm.checksum(y1[n]) for n in range(N)] == sums_x
    check_rows(y1, x, flat, True)
    check_rows(y1, x, seam_rows(True), True)
    g2 = lm.Guarded((N, npix, 1), device="cuda")
    y2 = _native.healpix_reorder(y1, nside, False, out=g2.view)
    torch.cuda.synchronize()
    g2.check("to_ring")
    assert [lm.checksum(y1[n]) for n in range(N)] == sums_x
    assert [lm.checksum(y2[n]) for n in range(N)] == sums_x
    check_rows(y2, y1, flat, False)
    check_rows(y2, y1, seam_rows(False), False)
    assert torch.equal(y2, x)
    print(f"peak device memory {torch.cuda.max_memory_allocated() / 1e9:.1f} GB")
