"""GPU tests of the rotation kernels (``dsph_healpix_rotate``, ``dsph_healpix_interp_table``) and of ``HealpyRotate`` on them
(``pytest -m gpu``).

The reference is ``healpix.get_interp_val`` in float64 (proven on the CPU in tests/test_interp_host.py), applied once per (nside,
rotation) as a stencil and shared by the cases.  VALUES are compared, never stencils entry by entry: at the symmetry rotations a
direction sits on a cell edge, where host and device may pick neighbouring cells with weight ~ 0 on the differing entry; the
interpolant is continuous, so the outputs agree.

Tolerance of every value comparison: 1e-6 max|x|.  Derived, not measured: four float32 weights, four products and three adds give
under 8 * 2^-24 * sum|w||x| ~ 5e-7 max|x| (the weights are non-negative and sum to 1); the float64 geometry differences add ~ 1e-12.

The kernel has two forms, F < 16 (a lane per pixel) and wider rows (stencils through LDS, lanes along the channels), each with 1, 2
or 4 floats per access by F and the alignment of the maps, blocks of 256 rows (more than one from nside 8), and a grid of
min(N, 65535) maps in y.  Outputs are NaN-filled views between sentinel bands (``large_map_ref.Guarded``)."""

import functools

import numpy as np
import pytest
import torch

import large_map_ref as lm
import rotate_ref as rr
from deepsphere import _native, healpix
from deepsphere.healpy_layers import HealpyChebyshev, HealpyRotate
from deepsphere.healpy_networks import HealpyGCNN
from helpers import offset_view

pytestmark = pytest.mark.gpu

NSIDES = (1, 2, 4, 8, 16, 32)
FS = (1, 3, 4, 16, 17, 64)
TOL = 1e-6


@functools.lru_cache(maxsize=None)
def host_stencil(nside, name):
    """(rows int64 [4, M], weights float64 [4, M]) of the named rotation on the full sky, computed once and never written."""
    rows, w = healpix.rotation_stencil(nside, rr.rotations(nside)[name])
    rows.setflags(write=False)
    w.setflags(write=False)
    return rows, w


def reference(x, nside, names):
    """The maps x (N, M, F) (numpy) rotated in float64 by the named rotations, one for all maps or one each."""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty_like(x)
    for n in range(x.shape[0]):
        rows, w = host_stencil(nside, names[n if len(names) > 1 else 0])
        out[n] = (x[n][rows] * w[:, :, None]).sum(axis=0)
    return out


def dev_rot(nside, names):
    R = np.stack([rr.rotations(nside)[k] for k in names])
    return torch.as_tensor(R[0] if len(names) == 1 else R).cuda().contiguous()


def maps(nside, F, N, seed=0):
    return torch.randn((N, 12 * nside * nside, F), generator=torch.Generator().manual_seed(1000 * nside + 10 * F + seed))


def run_case(nside, F, N, names, mis_x=0, mis_y=0):
    x = maps(nside, F, N)
    xd = offset_view(x, mis_x) if mis_x else x.cuda()
    before = lm.checksum(xd)
    g = lm.Guarded(tuple(x.shape), device="cuda", misalign=mis_y)
    out = _native.healpix_rotate(xd, nside, dev_rot(nside, names), out=g.view)
    torch.cuda.synchronize()
    what = f"nside {nside} F {F} N {N} {names}"
    assert out.data_ptr() == g.view.data_ptr()
    g.check(what)
    assert lm.checksum(xd) == before, what
    err = np.abs(out.cpu().numpy() - reference(x.numpy(), nside, names)).max()
    assert err <= TOL * float(x.abs().max()), (what, err)
    return x, out


CASES = sorted({(ns, F) for ns in NSIDES for F in (1, 4, 17)} | {(ns, F) for ns in (2, 8, 32) for F in FS})


@pytest.mark.parametrize("nside,F", CASES)
def test_kernel_against_get_interp_val(nside, F):
    names = list(rr.rotations(nside))
    assert len(names) == 10
    for name in names:
        run_case(nside, F, 1, (name,))
    run_case(nside, F, 3, ("zyz", "pole", "random1"))
    run_case(nside, F, 3, ("random2",))  # one rotation for the batch


@pytest.mark.parametrize("nside,F", [(ns, F) for ns in (2, 8, 32) for F in (1, 4, 16, 64)])
def test_symmetry_rotations_are_permutations(nside, F):
    for name, _, dst in rr.symmetry_cases(nside):
        x, out = run_case(nside, F, 2, (name,))
        err = np.abs(out.cpu().numpy() - rr.permuted(x.numpy(), dst)).max()
        assert err <= TOL * float(x.abs().max()), (name, err)


@pytest.mark.parametrize("nside,F,mis_x,mis_y", [(8, 1, 1, 0), (8, 1, 0, 2), (8, 2, 1, 0), (8, 2, 2, 2), (8, 2, 0, 1), (8, 4, 1, 0), (8, 4, 0, 2),
                                                 (8, 4, 2, 1), (8, 16, 1, 0), (8, 16, 0, 2), (8, 64, 2, 2)])
def test_views_off_16_byte_alignment(nside, F, mis_x, mis_y):
    """A view 4 or 8 bytes off on either side takes narrower accesses, in both forms of the kernel."""
    run_case(nside, F, 2, ("zyz", "random0"), mis_x, mis_y)


@pytest.mark.parametrize("F", (1, 16))
def test_maps_beyond_the_grid_take_a_second_trip(F):
    """N = 65,536 maps at nside 1: one more than the grid's y extent, with a rotation per map and with one for all."""
    nside, N = 1, 65536
    names = ("zyz", "pole", "random0")
    x = maps(nside, F, N)
    xd = x.cuda()
    R = np.stack([rr.rotations(nside)[k] for k in names])
    for per_map in (True, False):
        rot = torch.as_tensor(R[np.arange(N) % 3] if per_map else R[0]).cuda().contiguous()
        g = lm.Guarded(tuple(x.shape), device="cuda")
        out = _native.healpix_rotate(xd, nside, rot, out=g.view).cpu().numpy()
        g.check(f"F {F} per_map {per_map}")
        for k, name in enumerate(names if per_map else names[:1]):
            sel = slice(k, None, 3) if per_map else slice(None)
            rows, w = host_stencil(nside, name)
            xs = x.numpy()[sel].astype(np.float64)
            ref = sum(xs[:, rows[j]] * w[j][None, :, None] for j in range(4))
            assert np.abs(out[sel] - ref).max() <= TOL * float(x.abs().max())


def test_refusals_on_the_device():
    x = torch.zeros((1, 192, 2), device="cuda")
    R = torch.eye(3, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="overlap"):
        _native.healpix_rotate(x, 4, R, out=x)
    with pytest.raises(ValueError, match="rot lives on"):
        _native.healpix_rotate(x, 4, R.cpu())
    assert _native.healpix_rotate(torch.zeros((0, 192, 2), device="cuda"), 4, R).shape == (0, 192, 2)


@pytest.fixture(scope="module")
def footprint():
    ind = healpix.extend_indices(healpix.cap_indices(16, fraction=1 / 3), 16, 4)
    assert 0 < ind.size < 12 * 16 * 16
    return ind


@pytest.mark.parametrize("F", (1, 3, 4, 16, 17))
def test_partial_sky_is_the_zero_padded_full_sky(footprint, F):
    """Bit for bit: a source pixel outside the set contributes an explicit zero and nothing is renormalised."""
    nside, N = 16, 3
    ind, lut = healpix._device_lut(nside, footprint, torch.device("cuda"))
    x = torch.randn((N, footprint.size, F), generator=torch.Generator().manual_seed(40 + F)).cuda()
    full = torch.zeros((N, 12 * nside * nside, F), device="cuda")
    full[:, ind] = x
    for names in (("zyz", "mirror", "random0"), ("random1",)):  # a rotation per map, and n_rot == 1 shared over N = 3
        rot = dev_rot(nside, names)
        g = lm.Guarded(tuple(x.shape), device="cuda")
        part = _native.healpix_rotate(x, nside, rot, indices=ind, lut=lut, out=g.view)
        g.check(f"partial sky F {F}")
        whole = _native.healpix_rotate(full, nside, rot)
        assert torch.equal(part, whole[:, ind]), (F, names)
        assert bool(torch.isfinite(part).all()) and float(part.abs().max()) > 0
    # some stencils do reach outside the footprint (else this tests nothing)
    rows, _ = healpix.rotation_stencil(nside, rr.rotations(nside)["random1"], footprint)
    assert (rows < 0).any()


@pytest.mark.parametrize("nside", (1, 2, 4))
def test_table_against_the_host_stencil(nside):
    M = 12 * nside * nside
    for name, R in rr.rotations(nside).items():
        cols, vals = _native.healpix_interp_table(nside, torch.as_tensor(R).cuda())
        assert cols.shape == vals.shape == (M, 4) and cols.dtype == torch.int32 and vals.dtype == torch.float32
        c, v = cols.cpu().numpy().astype(np.int64), vals.cpu().numpy().astype(np.float64)
        assert c.min() >= 0 and c.max() < M
        assert (np.diff(np.sort(c, axis=1), axis=1) > 0).all(), f"{name}: a row holds a column twice"
        A = np.zeros((M, M))
        np.add.at(A, (np.repeat(np.arange(M), 4), c.reshape(-1)), v.reshape(-1))
        assert np.abs(A - rr.dense_stencil(nside, R)).max() <= TOL, name


@pytest.mark.parametrize("F", (1, 4, 17))
def test_table_through_ell_smooth_equals_the_kernel(footprint, F):
    nside = 16
    x = maps(nside, F, 2, seed=3).cuda()
    rot = dev_rot(nside, ("random0",))
    cols, vals = _native.healpix_interp_table(nside, rot)
    assert (np.diff(np.sort(cols.cpu().numpy(), axis=1), axis=1) > 0).all()
    err = (_native.ell_smooth(cols, vals, x) - _native.healpix_rotate(x, nside, rot)).abs().max()
    assert float(err) <= TOL * float(x.abs().max())
    # a partial-sky table: a source outside the set is (col = the row itself, val = 0), the padding of dsph_ell_smooth
    ind, lut = healpix._device_lut(nside, footprint, torch.device("cuda"))
    cols, vals = _native.healpix_interp_table(nside, rot, indices=ind, lut=lut)
    rows, w = healpix.rotation_stencil(nside, rr.rotations(nside)["random0"], footprint)
    c, v = cols.cpu().numpy(), vals.cpu().numpy()
    own = np.arange(footprint.size)[:, None]
    assert ((v != 0) | (c == own)).all() and c.min() >= 0 and c.max() < footprint.size
    xs = x[:, ind].contiguous()
    err = (_native.ell_smooth(cols, vals, xs) - _native.healpix_rotate(xs, nside, rot, indices=ind, lut=lut)).abs().max()
    assert float(err) <= TOL * float(x.abs().max())
    A = np.zeros((footprint.size, footprint.size))
    np.add.at(A, (np.repeat(np.arange(footprint.size), 4), c.reshape(-1).astype(np.int64)), v.reshape(-1).astype(np.float64))
    assert np.abs(A - rr.dense_stencil(nside, rr.rotations(nside)["random0"], footprint)).max() <= TOL


# ---- the layer ------------------------------------------------------------------------------------------------------------------

def test_layer_forward_equals_the_kernel(footprint):
    nside = 16
    R = rr.rotations(nside)["zyz"]
    x = maps(nside, 5, 3).cuda()
    layer = HealpyRotate(nside, rot=R)
    for mode in (layer.train, layer.eval):
        mode()
        assert torch.equal(layer(x), _native.healpix_rotate(x, nside, torch.as_tensor(R).cuda()))
    rots = torch.as_tensor(rr.random_rotations(3, 8))
    assert torch.equal(layer(x, rot=rots), _native.healpix_rotate(x, nside, rots.cuda()))
    assert torch.equal(layer(x, rot=rots[1].numpy()), _native.healpix_rotate(x, nside, rots[1].cuda().contiguous()))
    # partial sky; and the CPU path of the layer gives the same values
    ind, lut = healpix._device_lut(nside, footprint, torch.device("cuda"))
    part = HealpyRotate(nside, footprint, rot=R)
    xs = x[:, ind].contiguous()
    y = part(xs)
    assert torch.equal(y, _native.healpix_rotate(xs, nside, torch.as_tensor(R).cuda(), indices=ind, lut=lut))
    assert float((y.cpu() - part(xs.cpu())).abs().max()) <= TOL * float(xs.abs().max())


def test_layer_random_rotations():
    nside, N = 8, 4
    x = maps(nside, 2, 1).expand(N, -1, -1).contiguous().cuda()  # the same map in every sample
    a = HealpyRotate(nside, generator=torch.Generator().manual_seed(21))
    b = HealpyRotate(nside, generator=torch.Generator().manual_seed(21))
    ya, yb = a(x), b(x)
    assert torch.equal(ya, yb)
    assert all(not torch.equal(ya[0], ya[n]) for n in range(1, N)), "the samples of a batch got the same rotation"
    assert not torch.equal(a(x), ya), "a second call drew the same rotations"
    drawn = healpix.random_rotations(N, generator=torch.Generator().manual_seed(21)).cuda()
    assert torch.equal(ya, _native.healpix_rotate(x, nside, drawn))
    # a generator on the device, and none at all
    c = HealpyRotate(nside, generator=torch.Generator(device="cuda").manual_seed(22))(x)
    d = HealpyRotate(nside, generator=torch.Generator(device="cuda").manual_seed(22))(x)
    assert torch.equal(c, d) and not torch.equal(c, ya)
    assert HealpyRotate(nside)(x).shape == x.shape
    a.eval()
    assert a(x) is x


def test_layer_backward_is_the_transposed_stencil():
    nside, N, F = 4, 2, 3
    x = maps(nside, F, N).cuda()
    dy = maps(nside, F, N, seed=1).cuda()
    tol = TOL * float(dy.abs().max())
    rots = rr.random_rotations(N, 4)
    for layer, rot, mats in ((HealpyRotate(nside, rot=rots[0]), None, (rots[0], rots[0])),
                             (HealpyRotate(nside), torch.as_tensor(rots), (rots[0], rots[1])),
                             (HealpyRotate(nside), torch.as_tensor(rots[1]), (rots[1], rots[1]))):
        grads = []
        for _ in range(2):
            xg = x.clone().requires_grad_(True)
            (layer(xg, rot=rot) * dy).sum().backward()
            grads.append(xg.grad)
        assert torch.equal(grads[0], grads[1])
        for n in range(N):
            ref = rr.dense_stencil(nside, mats[n]).T @ dy[n].cpu().numpy().astype(np.float64)
            assert np.abs(grads[0][n].cpu().numpy() - ref).max() <= tol
    # partial sky
    ind = healpix.extend_indices(healpix.cap_indices(nside, fraction=1 / 3), nside, 2)
    layer = HealpyRotate(nside, ind, rot=rots[0])
    xg = x[:, torch.as_tensor(ind).cuda()].contiguous().requires_grad_(True)
    g = dy[:, torch.as_tensor(ind).cuda()].contiguous()
    (layer(xg) * g).sum().backward()
    ref = np.einsum("rm,nrf->nmf", rr.dense_stencil(nside, rots[0], ind), g.cpu().numpy().astype(np.float64))
    assert np.abs(xg.grad.cpu().numpy() - ref).max() <= tol
    # no gradient asked for: no table is built
    fixed = HealpyRotate(nside, rot=rots[0])
    fixed(x)
    assert not fixed._tables


def test_inside_a_network():
    nside = 8
    R = rr.rotations(nside)["zyz"]
    torch.manual_seed(11)
    net = HealpyGCNN(nside, None, [HealpyRotate(nside, rot=R), HealpyChebyshev(3, 4)])
    assert isinstance(net[0], HealpyRotate)
    x = maps(nside, 3, 2).cuda()
    with torch.no_grad():
        y = net(x)
        assert y.shape == (2, 12 * nside * nside, 4)
        assert torch.equal(y, net[1](_native.healpix_rotate(x, nside, torch.as_tensor(R).cuda())))


def test_graph_replay_of_a_fixed_rotation():
    """On the default queue settings."""
    nside = 16
    layer = HealpyRotate(nside, rot=rr.rotations(nside)["random0"])
    static_x = maps(nside, 4, 2).cuda()
    eager = layer(static_x).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        layer(static_x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_y = layer(static_x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_y, eager)
    other = maps(nside, 4, 2, seed=5).cuda()
    static_x.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_y, layer(other))
