"""GPU tests of the device graph build (``pytest -m gpu``): the k-NN kernel ``dsph_healpix_knn`` against brute force under the tie
rule of tests/graph_build_ref.py, the assembly behind it (``healpix.healpix_laplacian_ell``, ``healpix_adjacency_tables``,
``utils.prepare_ell``) against the host formulas applied to the kernel's own selection, and ``HealpyGCNN(build="device")`` end to end.

No test asks for the selection of ``healpix_graph(mode="knn")``: at a tied k-th neighbour either member of the mirror pair is right.
The kernel writes into sentinel-guarded buffers (``graph_build_ref.GuardedKnn``).  The full-sky sizes hold every place the kernel
can go wrong: polar caps, rings shorter than the window (nside 1 .. 4: whole rings), the 24 seven-neighbour corners, the
phi = 2 pi wrap; nside 64 and 128 every face border at a size where the window is a small part of the sphere, and M > 65535."""

import functools

import numpy as np
import pytest
import torch
from scipy import sparse

import graph_build_ref as gb
from deepsphere import _native, gnn_layers, healpix, utils
from deepsphere.healpy_layers import (HealpyBernstein, HealpyChebyshev, HealpyMonomial, HealpyPool, Healpy_ResidualLayer,
                                      Healpy_Transformer)
from deepsphere.healpy_networks import HealpyGCNN

pytestmark = pytest.mark.gpu


def cap16():
    return healpix.extend_indices(healpix.cap_indices(16, fraction=1 / 3), 16, 4)


def ragged32():
    """A random 30 % of the nside-8 super-pixels, at nside 32."""
    parents = np.sort(np.random.default_rng(5).choice(768, size=230, replace=False))
    return (parents[:, None] * 16 + np.arange(16)[None, :]).reshape(-1).astype(np.int64)


SETS = {"full": lambda nside: None, "cap16": lambda nside: cap16(), "ragged32": lambda nside: ragged32()}


@functools.lru_cache(maxsize=None)
def run_kernel(nside, k, which="full"):
    """The kernel on one set, into guarded buffers: -> (nbr, d2, ok) numpy, computed once per process and never written."""
    ind = SETS[which](nside)
    M = 12 * nside * nside if ind is None else ind.shape[0]
    g = gb.GuardedKnn(M, k)
    if ind is None:
        out = _native.healpix_knn(nside, k, device="cuda", out=g.out)
    else:
        out = _native.healpix_knn(nside, k, *healpix._device_lut(nside, ind, torch.device("cuda")), out=g.out)
    torch.cuda.synchronize()
    assert out[0].data_ptr() == g.out[0].data_ptr()
    g.check(f"nside {nside} k {k} {which}")
    return tuple(t.cpu().numpy() for t in out)


@functools.lru_cache(maxsize=2)
def distances(nside, which):
    return gb.brute_d2(gb.vectors(nside, SETS[which](nside)))


# ---- 1, 2: the selection on the full sky ----------------------------------------------------------------------------------------
FULL_CASES = [(1, 8)] + [(2, k) for k in (8, 20, 40)] + [(n, k) for n in (4, 8, 16) for k in (8, 20, 40, 60)]


@pytest.mark.parametrize("nside,k", FULL_CASES)
def test_full_sky_selection_is_valid(nside, k):
    nbr, d2, ok = run_kernel(nside, k)
    assert ok.all(), f"{int((ok == 0).sum())} rows of a full sky flagged"
    assert gb.selection_errors(gb.vectors(nside), nbr, d2, D=distances(nside, "full")) == []


@pytest.mark.parametrize("k", (20, 60))
def test_selection_across_all_faces(k):
    nbr, d2, ok = run_kernel(64, k)
    assert ok.all()
    assert gb.selection_errors_tree(gb.vectors(64), nbr, d2) == []


# ---- 3: partial sky ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (8, 20, 60))
@pytest.mark.parametrize("nside,which", [(16, "cap16"), (32, "ragged32")])
def test_partial_sky(nside, which, k):
    ind = SETS[which](nside)
    if which == "cap16":
        assert ind.shape[0] == 1152
    vec, D = gb.vectors(nside, ind), distances(nside, which)
    nbr, d2, ok = run_kernel(nside, k, which)
    good = np.nonzero(ok == 1)[0]
    assert gb.selection_errors(vec, nbr[good], d2[good], rows=good, D=D[good]) == []
    # a row whose k nearest in the set are its k nearest on the whole sphere is one the kernel must have guaranteed
    allvec = gb.vectors(nside)
    dk_set = np.sqrt(np.partition(D, k - 1, axis=1)[:, k - 1])
    dk_sky = np.empty_like(dk_set)
    for a in range(0, ind.shape[0], 512):
        Ds = ((allvec[None, :, :] - vec[a:a + 512, None, :]) ** 2).sum(axis=2)
        Ds[np.arange(Ds.shape[0]), ind[a:a + 512]] = np.inf
        dk_sky[a:a + 512] = np.sqrt(np.partition(Ds, k - 1, axis=1)[:, k - 1])
    interior = dk_set <= dk_sky * (1 + gb.EPS)
    assert interior.sum() > 0 and ok[interior].all(), f"{int((ok[interior] == 0).sum())} interior rows flagged"
    if which == "ragged32":
        assert (ok == 0).any()  # ... so the host completion below runs
    # the completed result is valid on every row
    cn, cd, completed = healpix.healpix_knn_device(nside, ind, k, device="cuda")
    assert completed == int((ok == 0).sum())
    assert gb.selection_errors(vec, cn.cpu().numpy(), cd.cpu().numpy(), D=D) == []


# ---- 4, 5, 6: from the selection to the tables -----------------------------------------------------------------------------------------
def csr_values_as_ell(L, shape):
    lens = np.diff(L.indptr)
    out = np.zeros(shape)
    out[np.repeat(np.arange(L.shape[0]), lens), np.arange(L.nnz) - np.repeat(L.indptr[:-1], lens)] = L.data
    return out


@pytest.mark.parametrize("nside,which,k", [(16, "full", 20), (16, "cap16", 20), (8, "full", 60), (16, "cap16", 8)])
def test_knn_assembly_is_the_hosts_on_the_same_selection(nside, which, k):
    ind = SETS[which](nside)
    nbr, d2, _ = healpix.healpix_knn_device(nside, ind, k, device="cuda")
    L = gb.host_laplacian_from_selection(nbr.cpu().numpy(), d2.cpu().numpy(), healpix.kernel_width(nside, k))
    cols, vals = healpix.healpix_laplacian_ell(nside, ind, k, "knn", device="cuda")
    assert cols.is_cuda and cols.dtype == torch.int32 and vals.dtype == torch.float64
    rc, _ = utils.csr_to_ell(L)
    cols, vals = cols.cpu().numpy(), vals.cpu().numpy()
    assert np.array_equal(cols, rc)
    np.testing.assert_allclose(vals, csr_values_as_ell(L, rc.shape), rtol=0, atol=1e-12)
    M = cols.shape[0]
    nz = vals != 0
    P = sparse.csr_matrix((np.ones(int(nz.sum())), (np.nonzero(nz)[0], cols[nz])), shape=(M, M))
    assert (P != P.T).nnz == 0
    assert nz.sum(axis=1).min() >= k + 1


@pytest.mark.parametrize("nside,which", [(8, "full"), (16, "cap16")])
def test_grid_assembly_is_the_hosts(nside, which):
    ind = SETS[which](nside)
    L = healpix.healpix_laplacian(nside, indices=ind, mode="grid")
    rc, _ = utils.csr_to_ell(L)
    cols, vals = healpix.healpix_laplacian_ell(nside, ind, mode="grid", device="cuda")
    assert np.array_equal(cols.cpu().numpy(), rc)
    np.testing.assert_allclose(vals.cpu().numpy(), csr_values_as_ell(L, rc.shape), rtol=0, atol=1e-12)


@pytest.mark.parametrize("nside,which,k,mode", [(8, "full", 20, "knn"), (16, "cap16", 8, "knn"), (16, "cap16", 8, "grid")])
def test_transformer_tables(nside, which, k, mode):
    ind = SETS[which](nside)
    if mode == "knn":
        nbr, d2, _ = healpix.healpix_knn_device(nside, ind, k, device="cuda")
        W = gb.host_graph_from_selection(nbr.cpu().numpy(), d2.cpu().numpy(), healpix.kernel_width(nside, k))
    else:
        W = healpix.healpix_graph(nside, ind, 8, "grid")
    t, tT = healpix.healpix_adjacency_tables(nside, ind, k, mode, device="cuda")
    assert tT is t and t.dtype == torch.int32 and np.array_equal(t.cpu().numpy(), utils.adjacency_to_ell(W))
    full = np.arange(12 * nside * nside) if ind is None else ind
    model = HealpyGCNN(nside, full, [Healpy_Transformer(key_dim=8, num_heads=2)], n_neighbors=k, graph_mode=mode, build="device")
    assert model[0].A is None and torch.equal(model[0].nbr, t) and model[0].nbrT is model[0].nbr
    with torch.no_grad():
        y = model(torch.randn(2, full.shape[0], 3, generator=torch.Generator().manual_seed(0)).cuda())
    assert y.shape == (2, full.shape[0], 16) and bool(torch.isfinite(y).all())


# ---- 7: past one grid row of workgroups ---------------------------------------------------------------------------------------------
def test_nside_128_build():
    k = 20
    nbr, d2, ok = run_kernel(128, k)  # (guards checked inside)
    assert ok.all() and nbr.shape == (196608, k)
    assert nbr.min() >= 0 and nbr.max() < 196608 and np.all(np.diff(d2, axis=1) >= 0)
    cols, vals = healpix.healpix_laplacian_ell(128, None, k, "knn", device="cuda")
    lens = (vals != 0).sum(dim=1)
    assert cols.shape[0] == 196608 and int(lens.min()) >= k + 1 and int(lens.max()) <= 2 * k + 1


# ---- 8: lmax ---------------------------------------------------------------------------------------------------------------------------
def test_prepare_ell_lmax_close_to_arpack():
    from scipy.sparse.linalg import eigsh

    L = healpix.healpix_laplacian(16, mode="grid")
    lam = eigsh(L, k=1, which="LM", return_eigenvectors=False)[0]
    cols, vals = healpix.healpix_laplacian_ell(16, mode="grid", device="cuda")
    pc, pv, lmax = utils.prepare_ell(cols, vals, 0.75)
    est = lmax / 1.02
    print(f"lanczos {est!r} arpack {lam!r} rel {abs(est - lam) / lam:.3g}")
    assert abs(est - lam) / lam < 2e-3 and est <= lam * (1 + 1e-5)  # the bounds of test_lanczos_lmax_close_to_arpack
    assert pc is cols and pv.dtype == torch.float32 and pv.is_cuda
    rc, rv = utils.csr_to_ell(utils.rescale_L(L, lmax=lmax, scale=0.75))
    assert np.array_equal(pc.cpu().numpy(), rc)
    np.testing.assert_allclose(pv.cpu().numpy(), rv, rtol=2e-7, atol=0)


# ---- 9, 10, 11: the model ------------------------------------------------------------------------------------------------------------
def graph_layers(model):
    out = []
    for layer in model:
        if isinstance(layer, gnn_layers.GCNN_ResidualLayer):
            out += [layer.layer1, layer.layer2]
        elif isinstance(layer, gnn_layers.Chebyshev):
            out.append(layer)
    return out


def test_full_model_on_shared_device_graphs():
    k = 20
    layers = [HealpyChebyshev(K=5, Fout=8, precision="fp32"), HealpyPool(1),
              Healpy_ResidualLayer("CHEBY", {"K": 3, "activation": "relu", "precision": "fp32"}, activation="relu"),
              HealpyMonomial(K=3, Fout=8, precision="fp32"), HealpyBernstein(K=3, Fout=4, precision="fp32")]
    model = HealpyGCNN(16, np.arange(3072), layers, n_neighbors=k, build="device")
    assert model.build_mode == "device"
    x = torch.randn(2, 3072, 3, generator=torch.Generator().manual_seed(1)).cuda()
    with torch.no_grad():
        y = model(x)
    assert y.shape == (2, 768, 4) and bool(torch.isfinite(y).all())
    first, res, mono, bern = model[0], model[2], model[3], model[4]
    # one graph per resolution: the layers at nside 8 share the column table, those of one scale the values too
    assert res.layer1._ell_cols is res.layer2._ell_cols is mono._ell_cols is bern._ell_cols
    assert res.layer1._ell_vals is res.layer2._ell_vals is bern._ell_vals and mono._ell_vals is not bern._ell_vals
    assert first._ell_cols is not bern._ell_cols and first._ell_cols.shape[0] == 3072
    assert all(layer.L is None for layer in graph_layers(model))
    assert res.layer1.lmax == bern.lmax == mono.lmax
    # every graph layer against a twin from the host formulas on the same selection and the same lmax
    for layer in graph_layers(model):
        nside = 16 if layer is first else 8
        nbr, d2, _ = healpix.healpix_knn_device(nside, None, k, device="cuda")
        L = gb.host_laplacian_from_selection(nbr.cpu().numpy(), d2.cpu().numpy(), healpix.kernel_width(nside, k))
        Lt = utils.rescale_L(L, lmax=layer.lmax, scale=layer._scale)
        Lt.sort_indices()
        tc, tv = utils.csr_to_ell(Lt.astype(np.float32))
        assert np.array_equal(layer._ell_cols, tc) and np.array_equal(layer._ell_vals, tv), type(layer).__name__
        twin = type(layer).from_prepared_ell(tc, tv, layer.K, lmax=layer.lmax, Fout=layer.Fout, activation=layer.activation,
                                             precision="fp32")
        xin = torch.randn(2, layer._M, layer._Fin, generator=torch.Generator().manual_seed(2)).cuda()
        twin.build(xin.shape)
        with torch.no_grad():
            twin.kernel.copy_(layer.kernel)
            assert torch.equal(layer(xin), twin(xin)), type(layer).__name__


def test_injected_arpack_lmax_reproduces_the_host_build(monkeypatch):
    spec = [HealpyChebyshev(K=5, Fout=8, precision="fp32", use_bias=True, activation="relu")]
    host = HealpyGCNN(16, np.arange(3072), spec, graph_mode="grid", build="host")
    prepare = utils.prepare_ell
    monkeypatch.setattr(utils, "prepare_ell", lambda cols, vals, scale, lmax=None, iters=64: prepare(cols, vals, scale, lmax=host[0].lmax))
    dev = HealpyGCNN(16, np.arange(3072), spec, graph_mode="grid", build="device")
    assert dev[0].lmax == host[0].lmax and dev[0].L is None
    assert np.array_equal(dev[0]._ell_cols, host[0]._ell_cols) and np.array_equal(dev[0]._ell_vals, host[0]._ell_vals)
    x = torch.randn(2, 3072, 4, generator=torch.Generator().manual_seed(3)).cuda()
    with torch.no_grad():
        yh = host(x)
        dev(x)
        dev.load_state_dict(host.state_dict())
        assert torch.equal(dev(x), yh)


def test_state_dict_round_trip_between_device_built_models():
    def make():
        return HealpyGCNN(8, np.arange(768), [HealpyChebyshev(K=3, Fout=8, use_bias=True), HealpyPool(1), HealpyMonomial(K=3, Fout=4)],
                          n_neighbors=8, build="device")

    a, b = make(), make()
    x = torch.randn(2, 768, 2, generator=torch.Generator().manual_seed(4)).cuda()
    with torch.no_grad():
        ya, yb = a(x), b(x)
        assert not torch.equal(ya, yb)  # (their own random weights)
        assert sorted(a.state_dict()) == sorted(b.state_dict()) and len(a.state_dict()) == 3
        b.load_state_dict(a.state_dict())
        assert torch.equal(b(x), ya)


def test_device_build_on_a_survey_footprint():
    ind = cap16()
    model = HealpyGCNN(16, ind, [HealpyChebyshev(K=3, Fout=4), HealpyPool(1), HealpyMonomial(K=3, Fout=4)], n_neighbors=20,
                       build="device")
    with torch.no_grad():
        y = model(torch.randn(2, ind.shape[0], 2, generator=torch.Generator().manual_seed(6)).cuda())
    assert y.shape == (2, ind.shape[0] // 4, 4) and bool(torch.isfinite(y).all())
    assert model[0]._ell_cols.shape[0] == 1152 and model[2]._ell_cols.shape[0] == 288
