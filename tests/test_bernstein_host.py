"""CPU tests of ``Bernstein`` / ``HealpyBernstein``: the coefficient matrix against the restated op sequence
(tests/bernstein_ref.py), constructor, lazy build, errors and the model builder.  Nothing is convolved without a GPU."""

import ctypes
import functools
from math import comb

import numpy as np
import pytest
import torch

import bernstein_ref as ref
from deepsphere import Bernstein as PackageBernstein
from deepsphere import HealpyBernstein as PackageHealpyBernstein
from deepsphere import _native, healpix
from deepsphere.gnn_layers import Bernstein, Chebyshev, GCNN_ResidualLayer, bernstein_to_chebyshev
from deepsphere.healpy_layers import HealpyBernstein, HealpyChebyshev, HealpyPool
from deepsphere.healpy_networks import HealpyGCNN
from oracle import cheb_oracle as orc


@functools.lru_cache(maxsize=None)
def nside4_layer():
    return Bernstein(healpix.healpix_laplacian(4), K=5, Fout=32, device="cpu")


@functools.lru_cache(maxsize=None)
def nside4_Lt():
    layer = nside4_layer()
    return ref.csr(layer._ell_cols, layer._ell_vals)


@pytest.mark.parametrize("K", [1, 2, 4, 5, 8])
def test_coefficients_reproduce_the_planes_of_the_op_sequence(K):
    Lt = nside4_Lt()
    x = np.random.default_rng(K).standard_normal((2, 192, 3))
    P = ref.planes(Lt, x, K)                       # (N, M, F, K + 1)
    T = orc.chebyshev_planes(Lt, x, K + 1)         # (K + 1, N, M, F)
    C = bernstein_to_chebyshev(K)
    assert C.shape == (K + 1, K + 1) and C.dtype == np.float64
    for i in range(K + 1):
        got = np.tensordot(C[i], T, axes=(0, 0))
        err = np.abs(got - P[..., i]).max() / np.abs(P[..., i]).max()
        print(f"K {K} plane {i}: {err:.2e}")
        assert err <= 1e-12
    # the reference's last plane is its plane K - 1 scaled again, not theta_K L~^K x
    theta_K = comb(K, K) / 2.0**K
    assert np.abs(P[..., K] - theta_K * P[..., K - 1]).max() <= 1e-15 * np.abs(P[..., K]).max()
    assert np.allclose(C[K], theta_K * C[K - 1], rtol=0, atol=1e-16)


def test_max_coefficient_by_order():
    got = {K: float(np.abs(bernstein_to_chebyshev(K)).max()) for K in (1, 2, 5, 10)}
    print(got)
    assert got[1] == 1.0 and got[2] == 1.125 and abs(got[5] - 5.41) < 0.01 and abs(got[10] - 94.08) < 0.01


@pytest.mark.parametrize("K,Fin,Fout", [(5, 1, 32), (2, 7, None), (1, 16, 4)])
def test_build_shapes_and_default_initialiser(K, Fin, Fout):
    base = nside4_layer()
    layer = Bernstein.from_prepared_ell(base._ell_cols, base._ell_vals, K, Fout=Fout, use_bias=True, use_bn=True, device="cpu")
    assert isinstance(layer, Chebyshev) and layer.K == K and layer._n_terms == K + 1 and layer.kernel is None
    torch.manual_seed(0)
    layer.build((2, 192, Fin))
    fo = Fin if Fout is None else Fout
    assert tuple(layer.kernel.shape) == ((K + 1) * Fin, fo) and tuple(layer.bias.shape) == (1, 1, fo)
    std = np.sqrt(6.0 / (Fin + fo))
    assert layer._default_stddev(Fin, fo) == pytest.approx(std)
    k = layer.kernel.detach().numpy()
    assert np.abs(k).max() <= 2.0 * std * (1 + 1e-6)       # truncated at two standard deviations
    if k.size >= 64:
        assert 0.6 * std < k.std() < 1.0 * std             # (a normal truncated at 2 sigma has 0.88 of its stddev)
    # the coefficient matrix is no parameter and is not saved
    assert set(layer.state_dict()) == {"kernel", "bias", "bn.running_mean", "bn.running_var", "bn.num_batches_tracked"}
    assert [n for n, _ in layer.named_parameters()] == ["kernel", "bias"]


def test_initializer_and_attributes_follow_the_reference():
    L = healpix.healpix_laplacian(4)
    layer = Bernstein(L, 4, Fout=3, initializer=lambda t: torch.nn.init.constant_(t, 0.25), activation="linear", n_matmul_splits=2,
                      device="cpu")
    assert layer.L is L and layer.K == 4 and layer.Fout == 3 and layer.n_matmul_splits == 2 and layer.activation is None
    assert not layer.use_bias and not layer.use_bn
    layer.build((5, 192, 7))
    assert tuple(layer.kernel.shape) == (35, 3) and float(layer.kernel.detach().min()) == float(layer.kernel.detach().max()) == 0.25


def test_errors():
    L = healpix.healpix_laplacian(4)
    with pytest.raises(ValueError, match="Could not find activation"):
        Bernstein(L, 5, activation="no_such_activation")
    with pytest.raises(ValueError, match="K must be at least 1"):
        Bernstein(L, 0)
    with pytest.raises(ValueError, match="K must be at least 1"):
        bernstein_to_chebyshev(0)
    with pytest.raises(IOError):
        GCNN_ResidualLayer("BERN", {"L": L, "K": 5})
    # dsph_basis_change refuses before any device call (made-up addresses 8 TiB apart that nothing dereferences): an output over
    # an input; and, at 2^40 elements, the grid of a call whose pointers allow 2 floats (8-byte aligned) or 1 float (4-byte
    # aligned) per access -- 2^31 and 2^32 workgroups, where 4 floats per access are 2^30 and would launch
    lib = _native.lib()
    W, C, O = 1 << 44, 1 << 43, 1 << 45

    def change(w=W, c=C, o=O, Fin=4, Fout=8, Kp=3):
        rc = lib.dsph_basis_change(ctypes.c_void_p(w), ctypes.c_void_p(c), ctypes.c_void_p(o), Fin, Fout, Kp, 0, 0, ctypes.c_void_p())
        return rc, _native.last_error()

    nbytes = 4 * 3 * 8 * 4
    for kw, text in [(dict(o=W), "w and w_out overlap"), (dict(o=W + 4), "w and w_out overlap"), (dict(o=W + nbytes - 4), "w and w_out overlap"),
                     (dict(o=W - nbytes + 4), "w and w_out overlap"), (dict(c=O - 32), "coeff and w_out overlap"),
                     (dict(c=O + nbytes - 4), "coeff and w_out overlap")]:
        rc, msg = change(**kw)
        assert rc == -1 and text in msg, (kw, rc, msg)
    big = dict(Fin=1 << 24, Fout=1 << 10, Kp=64)
    for kw, text in [(dict(w=W + 8), "2147483648 workgroups"), (dict(o=O + 8), "2147483648 workgroups"), (dict(w=W + 4), "4294967296 workgroups"),
                     (dict(w=W + 8, o=O + 4), "4294967296 workgroups")]:
        rc, msg = change(**kw, **big)
        assert rc == -3 and text in msg, (kw, rc, msg)


def test_exports():
    import deepsphere
    from deepsphere import gnn_layers, healpy_layers

    assert PackageBernstein is Bernstein and PackageHealpyBernstein is HealpyBernstein
    assert "Bernstein" in gnn_layers.__all__ and "HealpyBernstein" in healpy_layers.__all__
    assert issubclass(HealpyBernstein, HealpyChebyshev) and deepsphere.Bernstein.__mro__[1] is Chebyshev


def test_model_builder_holds_two_bernstein_layers():
    model = HealpyGCNN(4, np.arange(192), [HealpyBernstein(K=5, Fout=32), HealpyPool(1), HealpyBernstein(K=5, Fout=32)])
    assert len(model) == 3 and type(model[0]) is Bernstein and type(model[2]) is Bernstein and isinstance(model[1], HealpyPool)
    assert model[0]._M == 192 and model[2]._M == 48 and model[0].K == 5 and model[2].Fout == 32
    assert model.nside_out == 2 and np.array_equal(model.indices_out, np.arange(48))
