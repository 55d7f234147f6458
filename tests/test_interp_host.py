"""CPU tests of the point-to-pixel half of HEALPix in ``healpix.py`` (``ang2pix``, ``vec2pix``, ``pix2ang``, ``get_interp_weights``,
``get_interp_val``, ``rotation_matrix``, ``random_rotations``), of ``HealpyRotate`` on CPU tensors and of the refusals of
``_native.healpix_rotate`` / ``healpix_interp_table``.  They make the numpy functions the proven reference of the GPU tests
(tests/test_gpu_rotate.py): round trips, the weights at pixel centres and at hand-picked directions, the symmetries of the grid
(independent of the implementation: exact pixel permutations) and a smooth field whose interpolation error must fall with nside."""

import numpy as np
import pytest
import torch

import deepsphere
import rotate_ref as rr
from deepsphere import _native, healpix, healpy_layers
from deepsphere.healpy_layers import HealpyRotate

EPS = np.finfo(np.float64).eps


@pytest.mark.parametrize("nside", (1, 2, 4, 16, 64))
def test_round_trips(nside):
    p = np.arange(12 * nside * nside, dtype=np.int64)
    for nest in (True, False):
        theta, phi = healpix.pix2ang(nside, p, nest=nest)
        assert theta.min() > 0 and theta.max() < np.pi and phi.min() >= 0 and phi.max() < 2 * np.pi
        assert np.array_equal(healpix.ang2pix(nside, theta, phi, nest=nest), p)
    v = healpix.pix2vec(nside, p)
    assert np.array_equal(healpix.vec2pix(nside, v[:, 0], v[:, 1], v[:, 2]), p)
    assert np.array_equal(healpix.vec2pix(nside, 3 * v[:, 0], 3 * v[:, 1], 3 * v[:, 2], nest=False), healpix.nest2ring(nside, p))
    theta, phi = healpix.pix2ang(nside, p)
    assert np.abs(np.cos(theta) - v[:, 2]).max() < 4 * EPS and np.abs(np.sin(theta) * np.cos(phi) - v[:, 0]).max() < 8 * EPS


@pytest.mark.parametrize("nside", (1, 2, 4, 16, 64))
def test_weights_at_a_pixels_own_centre(nside):
    p = np.arange(12 * nside * nside, dtype=np.int64)
    for nest in (True, False):
        pix, w = healpix.get_interp_weights(nside, p, nest=nest)
        own = pix == p[None]
        assert np.array_equal(own.sum(axis=0), np.ones_like(p))
        assert np.abs(w[own] - 1.0).max() < 1e-12 and np.abs(w[~own]).max() < 1e-12


def hand_picked(nside):
    """(theta, phi): the poles, inside the first and the last ring, phi at and around the 2 pi seam, z = +-2/3."""
    t1 = healpix.pix2ang(nside, np.array([0]))[0][0]  # colatitude of the first ring
    thetas = [0.0, np.pi, 0.3 * t1, 0.999 * t1, np.pi - 0.3 * t1, np.pi - 0.999 * t1, np.arccos(2 / 3), np.arccos(-2 / 3), t1, np.pi - t1,
              0.5 * np.pi, 1.0]
    phis = [0.0, 2 * np.pi - 1e-17, -1e-17, 2 * np.pi, 0.25 * np.pi, 0.5 * np.pi, np.nextafter(2 * np.pi, 0), 5.0, -3.0, 7.0]
    t, f = np.meshgrid(thetas, phis, indexing="ij")
    return t.reshape(-1), f.reshape(-1)


@pytest.mark.parametrize("nside", (1, 2, 8, 32))
def test_weights_in_general(nside):
    rng = np.random.default_rng(100 + nside)
    v = rng.standard_normal((10000, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    theta = np.concatenate([np.arccos(v[:, 2]), hand_picked(nside)[0]])
    phi = np.concatenate([np.arctan2(v[:, 1], v[:, 0]), hand_picked(nside)[1]])
    npix = 12 * nside * nside
    for nest in (True, False):
        pix, w = healpix.get_interp_weights(nside, theta, phi, nest=nest)
        assert pix.shape == w.shape == (4, theta.size) and pix.dtype == np.int64 and w.dtype == np.float64
        assert pix.min() >= 0 and pix.max() < npix
        assert np.abs(w.sum(axis=0) - 1.0).max() <= 4 * EPS
        assert w.min() >= -1e-12
        s = np.sort(pix, axis=0)
        assert (np.diff(s, axis=0) > 0).all(), "a row holds a pixel twice"
    # the interpolant reproduces constants and is continuous across the 2 pi seam
    a = healpix.get_interp_val(np.arange(npix, dtype=np.float64), theta, -1e-17 * np.ones_like(theta))
    b = healpix.get_interp_val(np.arange(npix, dtype=np.float64), theta, np.zeros_like(theta))
    assert np.abs(a - b).max() <= 1e-11 * npix
    # scalars and 2-d arrays of directions keep their shape behind the leading 4
    assert healpix.get_interp_weights(nside, 1.0, 2.0)[0].shape == (4,)
    assert healpix.get_interp_weights(nside, theta[:6].reshape(2, 3), phi[:6].reshape(2, 3))[1].shape == (4, 2, 3)
    with pytest.raises(ValueError, match="theta"):
        healpix.get_interp_weights(nside, -0.1, 0.0)


@pytest.mark.parametrize("nside", (8, 16, 64))
def test_the_seam_wraps_both_positions(nside):
    """A 90 degree rotation about z turns pixel centres with phi = 3 pi / 2 onto phi = -1e-17 or so, which reduces to exactly 2 pi:
    the first position is then the ring length and must wrap like the second."""
    theta = healpix.pix2ang(nside, np.arange(12 * nside * nside))[0]
    theta = np.unique(theta)
    for phi in (-1e-17, 2 * np.pi - 1e-17, 2 * np.pi):
        pix, w = healpix.get_interp_weights(nside, theta, np.full_like(theta, phi))
        pix0, w0 = healpix.get_interp_weights(nside, theta, np.zeros_like(theta))
        assert np.array_equal(pix, pix0) and np.abs(w - w0).max() < 1e-12


@pytest.mark.parametrize("nside", (2, 4, 8, 16, 32))
def test_symmetries_are_exact_permutations(nside):
    npix = 12 * nside * nside
    m = np.random.default_rng(nside).standard_normal(npix)
    for name, R, dst in rr.symmetry_cases(nside):
        theta, phi = rr.source_angles(nside, R)
        y = healpix.get_interp_val(m, theta, phi)
        err = np.abs(y - rr.permuted(m, dst)).max()
        assert err <= 1e-11 * np.abs(m).max(), (name, err)
        rows, w = healpix.rotation_stencil(nside, R)
        assert np.array_equal(y, (m[rows] * w).sum(axis=0))
    k = np.stack([m, 2 * m])  # (k, npix) maps
    theta, phi = rr.source_angles(nside, rr.MIRROR)
    assert np.array_equal(healpix.get_interp_val(k, theta, phi)[1], 2 * healpix.get_interp_val(m, theta, phi))


def test_smooth_field_error_falls_with_nside():
    """A wrong ring or a wrong shift flag gives an error that does not fall with nside.  Measured: 0.25, 0.26, 0.25, 0.22, 0.17
    over nside for nside 4 .. 64."""
    R = healpix.rotation_matrix(*rr.ZYZ)
    errs = []
    for nside in (4, 8, 16, 32, 64):
        v = healpix.pix2vec(nside)
        theta, phi = rr.source_angles(nside, R)
        y = healpix.get_interp_val(rr.field(v), theta, phi)
        errs.append(np.abs(y - rr.field(v @ R)).max())
        print(f"nside {nside}: error {errs[-1]:.3e} = {errs[-1] * nside:.3f} / nside")
        assert errs[-1] < 0.5 / nside
    assert all(b < a for a, b in zip(errs, errs[1:]))


def test_rotation_matrix_and_random_rotations():
    R = healpix.rotation_matrix(*rr.ZYZ)
    assert R.dtype == np.float64 and np.abs(R.T @ R - np.eye(3)).max() < 4 * EPS and abs(np.linalg.det(R) - 1) < 4 * EPS
    assert np.abs(healpix.rotation_matrix(0.5 * np.pi, 0, 0) - rr.z_rotation(1)).max() < 2 * EPS
    assert np.abs(healpix.rotation_matrix(0, 0, 0.5 * np.pi) - rr.z_rotation(1)).max() < 2 * EPS
    assert np.abs(healpix.rotation_matrix(0, 0.5 * np.pi, 0) @ [0, 0, 1] - [1, 0, 0]).max() < 2 * EPS  # Ry takes z to x
    a = healpix.random_rotations(1000, generator=torch.Generator().manual_seed(3))
    b = healpix.random_rotations(1000, generator=torch.Generator().manual_seed(3))
    assert a.dtype == torch.float64 and a.shape == (1000, 3, 3) and torch.equal(a, b)
    assert (a.transpose(1, 2) @ a - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-14
    assert (torch.linalg.det(a) - 1).abs().max() < 1e-14
    # uniform on SO(3): the image of z is uniform on the sphere (mean 0, every coordinate's variance 1 / 3)
    z = a[:, :, 2]
    assert z.mean(0).abs().max() < 0.08 and (z.var(0) - 1 / 3).abs().max() < 0.05
    assert healpix.random_rotations(0).shape == (0, 3, 3)


def test_exports():
    for name in ("ang2pix", "vec2pix", "pix2ang", "get_interp_weights", "get_interp_val", "rotation_matrix", "random_rotations"):
        assert name in healpix.__all__ and callable(getattr(healpix, name))
    assert deepsphere.HealpyRotate is HealpyRotate and "HealpyRotate" in healpy_layers.__all__
    for name, nargs in (("dsph_healpix_rotate", 12), ("dsph_healpix_interp_table", 9)):
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == nargs


def test_binding_refuses_before_it_touches_the_gpu():
    x = torch.zeros(1, 192, 2)
    R = torch.eye(3, dtype=torch.float64)
    bad = [
        (dict(x=x, nside=3, rot=R), "power of two"),
        (dict(x=x, nside=16384, rot=R), "8192"),
        (dict(x=x.double(), nside=4, rot=R), "float32"),
        (dict(x=x.transpose(1, 2), nside=4, rot=R), "contiguous"),
        (dict(x=x[:, :-1], nside=4, rot=R), "191"),
        (dict(x=x, nside=4, rot=R.float()), "float64"),
        (dict(x=x, nside=4, rot=torch.zeros(2, 3, 3, dtype=torch.float64)), r"\[N = 1, 3, 3\]"),
        (dict(x=x, nside=4, rot=R.numpy()), "float64 tensor"),
        (dict(x=x, nside=4, rot=R, indices=torch.arange(192)), "come together"),
        (dict(x=x, nside=4, rot=R, out=torch.zeros(1, 192, 1)), "out must be"),
        (dict(x=x, nside=4, rot=R), "HIP tensor"),
    ]
    for kwargs, match in bad:
        with pytest.raises(ValueError, match=match):
            _native.healpix_rotate(**kwargs)
    for kwargs, match in [(dict(nside=5, rot=R), "power of two"), (dict(nside=4, rot=R.float()), "float64"),
                          (dict(nside=4, rot=torch.zeros(1, 3, 3, dtype=torch.float64)), r"\[3, 3\]"),
                          (dict(nside=4, rot=R, lut=torch.zeros(192, dtype=torch.int32)), "come together"),
                          (dict(nside=4, rot=R, device="cpu"), "HIP device")]:
        with pytest.raises(ValueError, match=match):
            _native.healpix_interp_table(**kwargs)


def test_c_entry_points_refuse_bad_arguments():
    import ctypes

    lib = _native.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    q = p + 256
    B, U = -1, -3

    def refused(rc, code, *words):
        assert rc == code, (rc, _native.last_error())
        for wd in words:
            assert wd in _native.last_error(), _native.last_error()

    refused(lib.dsph_healpix_rotate(None, q, 1, 4, 1, p, 1, None, None, 192, 0, None), B, "healpix_rotate", "NULL")
    refused(lib.dsph_healpix_rotate(p, q, 1, 4, 1, None, 1, None, None, 192, 0, None), B, "healpix_rotate", "NULL")
    refused(lib.dsph_healpix_rotate(p, q, 1, 3, 1, p, 1, None, None, 108, 0, None), B, "power of two")
    refused(lib.dsph_healpix_rotate(p, q, 1, 16384, 1, p, 1, None, None, 12 * 16384**2, 0, None), U, "8192")
    refused(lib.dsph_healpix_rotate(p, q, 1, 4, 1, p, 1, p, None, 192, 0, None), B, "come together")
    refused(lib.dsph_healpix_rotate(p, q, 1, 4, 1, p, 1, None, None, 191, 0, None), B, "without indices")
    refused(lib.dsph_healpix_rotate(p, q, 1, 4, 1, p, 1, p, p, 193, 0, None), B, "M = 193")
    refused(lib.dsph_healpix_rotate(p, q, 1, 4, 0, p, 1, None, None, 192, 0, None), B, "F = 0")
    refused(lib.dsph_healpix_rotate(p, q, -1, 4, 1, p, 1, None, None, 192, 0, None), B, "N = -1")
    refused(lib.dsph_healpix_rotate(p, q, 3, 4, 1, p, 2, None, None, 192, 0, None), B, "n_rot = 2")
    refused(lib.dsph_healpix_rotate(p, q, 1, 4, 1, p + 4, 1, None, None, 192, 0, None), B, "8-byte")
    refused(lib.dsph_healpix_rotate(p, p + 16, 1, 4, 1, q, 1, None, None, 192, 0, None), B, "overlap")
    refused(lib.dsph_healpix_interp_table(4, None, None, None, 192, p, q, 0, None), B, "healpix_interp_table", "NULL")
    refused(lib.dsph_healpix_interp_table(4, p, None, None, 192, None, q, 0, None), B, "NULL")
    refused(lib.dsph_healpix_interp_table(6, p, None, None, 432, p, q, 0, None), B, "power of two")
    refused(lib.dsph_healpix_interp_table(4, p, None, p, 100, p, q, 0, None), B, "come together")
    refused(lib.dsph_healpix_interp_table(4, p, None, None, 100, p, q, 0, None), B, "without indices")


def test_layer_argument_checks_and_modes():
    with pytest.raises(ValueError, match="power of two"):
        HealpyRotate(12)
    with pytest.raises(ValueError, match="8192"):
        HealpyRotate(16384)
    with pytest.raises(ValueError, match="random"):
        HealpyRotate(4, rot="uniform")
    with pytest.raises(ValueError, match="rotation matrix"):
        HealpyRotate(4, rot=np.zeros((3, 3)))
    with pytest.raises(ValueError, match="rotation matrix"):
        HealpyRotate(4, rot=np.diag([1.0, 1.0, -1.0]))  # a reflection
    with pytest.raises(ValueError, match="rotation matrix"):
        HealpyRotate(4, rot=np.eye(4))
    with pytest.raises(ValueError, match="sorted unique"):
        HealpyRotate(4, indices=[3, 1, 2])
    layer = HealpyRotate(4)
    assert not hasattr(layer, "p") and not hasattr(layer, "Fout")
    x = torch.randn(2, 192, 3, generator=torch.Generator().manual_seed(0))
    with pytest.raises(ValueError, match=r"191.*192"):
        layer(x[:, :-1])
    with pytest.raises(ValueError, match=r"\[N = 2, 3, 3\]"):
        layer(x, rot=torch.zeros(3, 3, 3, dtype=torch.float64))
    layer.eval()
    assert layer(x) is x  # random rotations are not drawn in eval() mode: the identity, the input object itself
    assert layer.call == layer.forward


@pytest.mark.parametrize("dtype", (torch.float32, torch.float64))
def test_layer_on_cpu_tensors(dtype):
    nside, N, F = 4, 3, 2
    x = torch.randn(N, 12 * nside * nside, F, generator=torch.Generator().manual_seed(1)).to(dtype)
    tol = (1e-6 if dtype == torch.float32 else 1e-12) * float(x.abs().max())
    R = healpix.rotation_matrix(*rr.ZYZ)
    fixed = HealpyRotate(nside, rot=R)
    for mode in (fixed.train, fixed.eval):  # a given rotation is applied in both modes
        mode()
        y = fixed(x)
        assert y.dtype == dtype and np.abs(y.numpy() - rr.rotate_map64(x.numpy(), nside, R)).max() <= tol
    # an explicit rotation overrides the setting: one per sample
    rots = rr.random_rotations(N, 5)
    y = fixed(x, rot=rots)
    assert np.abs(y.numpy() - rr.rotate_map64(x.numpy(), nside, rots)).max() <= tol
    assert np.abs(HealpyRotate(nside).eval()(x, rot=R).numpy() - rr.rotate_map64(x.numpy(), nside, R)).max() <= tol
    # rot="random": reproducible from the generator's seed, a rotation per sample
    a = HealpyRotate(nside, generator=torch.Generator().manual_seed(9))(x)
    b = HealpyRotate(nside, generator=torch.Generator().manual_seed(9))(x)
    drawn = healpix.random_rotations(N, generator=torch.Generator().manual_seed(9)).numpy()
    assert torch.equal(a, b) and np.abs(a.numpy() - rr.rotate_map64(x.numpy(), nside, drawn)).max() <= tol
    same = x[:1].expand(N, -1, -1).contiguous()
    c = HealpyRotate(nside, generator=torch.Generator().manual_seed(9))(same)
    assert not torch.equal(c[0], c[1]) and not torch.equal(c[1], c[2])
    # the symmetry rotations are permutations
    for name, Rs, dst in rr.symmetry_cases(nside):
        assert np.abs(HealpyRotate(nside, rot=Rs)(x).numpy() - rr.permuted(x.numpy(), dst)).max() <= tol, name


def test_layer_gradient_and_partial_sky_on_cpu():
    nside = 4
    ind = healpix.extend_indices(healpix.cap_indices(nside, fraction=1 / 3), nside, 2)
    R = healpix.rotation_matrix(*rr.ZYZ)
    x = torch.randn(2, ind.size, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(2), requires_grad=True)
    g = torch.randn(2, ind.size, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    layer = HealpyRotate(nside, ind, rot=R)
    y = layer(x)
    # the rotated zero-padded full-sky map, read at the footprint
    full = np.zeros((2, 12 * nside * nside, 3))
    full[:, ind] = x.detach().numpy()
    assert np.abs(y.detach().numpy() - rr.rotate_map64(full, nside, R)[:, ind]).max() < 1e-12
    (y * g).sum().backward()
    A = rr.dense_stencil(nside, R, ind)
    assert np.abs(x.grad.numpy() - np.einsum("rm,nrf->nmf", A, g.numpy())).max() < 1e-12
    assert (A.sum(axis=1) < 1 - 1e-6).any(), "no stencil of this footprint reaches outside it: the case tests nothing"
