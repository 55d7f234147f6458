"""References for the rotation tests (tests/test_interp_host.py, tests/test_gpu_rotate.py; not collected by pytest): the symmetry
rotations of the HEALPix grid with their exact pixel permutations, the smooth test field, the named rotations, and the float64
rotation of a map through ``healpix.get_interp_val`` (proven on the CPU against the permutations and the smooth field)."""

import functools

import numpy as np

from deepsphere import healpix

# the smooth field f(v) = a . v + v^T Q v and the rotation it is turned by
FIELD_A = np.array([0.3, -0.5, 0.8])
FIELD_Q = np.array([[0.5, 0.2, -0.3], [0.2, -0.7, 0.4], [-0.3, 0.4, 0.2]])
ZYZ = (0.3, 1.1, -2.0)


def field(v):
    return v @ FIELD_A + np.einsum("ni,ij,nj->n", v, FIELD_Q, v)


def z_rotation(q):
    """Rotation by q * 90 degrees about z, exact entries."""
    c, s = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[q & 3]
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


MIRROR = np.diag([1.0, -1.0, -1.0])  # rotation by 180 degrees about x


@functools.lru_cache(maxsize=None)
def z_permutation(nside, q):
    """dst[p]: where the rotation by q * 90 degrees about z takes pixel p -- the face moves on by q inside its row of four, (ix, iy)
    stay: y[dst] = x."""
    ix, iy, face = healpix.nest2xyf(nside, np.arange(12 * nside * nside, dtype=np.int64))
    dst = healpix.xyf2nest(nside, ix, iy, (face & ~3) | ((face + q) & 3))
    dst.setflags(write=False)
    return dst


@functools.lru_cache(maxsize=None)
def mirror_permutation(nside):
    """dst[p]: the pixel whose centre is nearest to MIRROR v(p) (the grid is symmetric under it: the distance is rounding)."""
    from scipy.spatial import cKDTree

    v = healpix.pix2vec(nside)
    d, dst = cKDTree(v).query(v @ MIRROR.T)
    assert d.max() < 1e-12 and np.array_equal(np.sort(dst), np.arange(v.shape[0]))
    dst = dst.astype(np.int64)
    dst.setflags(write=False)
    return dst


def symmetry_cases(nside):
    """(name, rotation, dst) of the four symmetry rotations: the rotated map is exactly y[dst] = x."""
    return [(f"z{90 * q}", z_rotation(q), z_permutation(nside, q)) for q in (1, 2, 3)] + [("mirror", MIRROR, mirror_permutation(nside))]


def permuted(m, dst):
    """y with y[..., dst, :] = m along the pixel axis (axis -2 of (N, M, F), axis 0 of (M,))."""
    out = np.empty_like(m)
    if m.ndim == 1:
        out[dst] = m
    else:
        out[..., dst, :] = m
    return out


def pole_rotation(nside, pix):
    """A rotation with R^T v(pix) = north pole; the antipodal pixel (the grid is point-symmetric) then reads the south pole."""
    theta, phi = healpix.pix2ang(nside, np.array([pix]))
    return healpix.rotation_matrix(float(phi[0]), float(theta[0]), 0.0)


def random_rotations(n, seed):
    import torch

    return healpix.random_rotations(n, generator=torch.Generator().manual_seed(seed)).numpy()


@functools.lru_cache(maxsize=None)
def rotations(nside):
    """name -> matrix: the rotations the kernel is compared under (one dict per nside, shared: not to be written)."""
    out = {"identity": np.eye(3)}
    out.update({name: R for name, R, _ in symmetry_cases(nside)})
    out["zyz"] = healpix.rotation_matrix(*ZYZ)
    out["pole"] = pole_rotation(nside, (5 * nside * nside) // 2 + 1 if nside > 1 else 5)
    for i, R in enumerate(random_rotations(3, 17)):
        out[f"random{i}"] = R
    return out


def source_angles(nside, R, indices=None):
    """(theta, phi) of R^T v(p) for the pixels of the set."""
    u = healpix.pix2vec(nside, indices) @ np.asarray(R, dtype=np.float64)
    return np.arctan2(np.hypot(u[:, 0], u[:, 1]), u[:, 2]), np.arctan2(u[:, 1], u[:, 0])


def rotate_map64(x, nside, rot):
    """The full-sky maps x (N, npix, F) rotated in float64 through ``get_interp_val``; rot [3, 3] or [N, 3, 3]."""
    x = np.asarray(x, dtype=np.float64)
    rot = np.asarray(rot, dtype=np.float64).reshape(-1, 3, 3)
    out = np.empty_like(x)
    for n in range(x.shape[0]):
        theta, phi = source_angles(nside, rot[n if rot.shape[0] > 1 else 0])
        out[n] = healpix.get_interp_val(x[n].T, theta, phi).T
    return out


def dense_stencil(nside, R, indices=None):
    """The rotation as a dense float64 matrix [M, M] from the host stencil (y = A x)."""
    rows, w = healpix.rotation_stencil(nside, R, indices)
    M = rows.shape[1]
    A = np.zeros((M, M))
    for j in range(4):
        keep = rows[j] >= 0
        np.add.at(A, (np.nonzero(keep)[0], rows[j][keep]), w[j][keep])
    return A
