"""CPU tests of the device graph build: the argument checks of ``_native.healpix_knn`` and of ``HealpyGCNN(build=...)``, the reference
helpers of tests/graph_build_ref.py against ``healpix.healpix_graph`` where no tie is in play, and everything between a neighbour
selection and the prepared table (``healpix.DeviceGraph``, ``healpix_laplacian_ell``, ``utils.prepare_ell``) on torch CPU tensors --
the k-NN kernel replaced by the brute-force search, which is all the assembly needs.  The kernel itself: tests/test_gpu_graph_build.py."""

import numpy as np
import pytest
import torch

import graph_build_ref as gb
from deepsphere import _native, healpix, utils
from deepsphere.healpy_layers import HealpyChebyshev
from deepsphere.healpy_networks import HealpyGCNN


def cap16():
    return healpix.extend_indices(healpix.cap_indices(16, fraction=1 / 3), 16, 4)


# ---- argument checks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kwargs,match", [
    (dict(nside=3, k=8), "power of two"),
    (dict(nside=0, k=8), "power of two"),
    (dict(nside=16384, k=8), "8192"),
    (dict(nside=8, k=0), "1 .. 64"),
    (dict(nside=8, k=65), "1 .. 64"),
    (dict(nside=1, k=20), "M > k"),
    (dict(nside=1, k=12), "M > k"),
    (dict(nside=8, k=8, indices=torch.arange(40)), "come together"),
    (dict(nside=8, k=8, lut=torch.zeros(768, dtype=torch.int32)), "come together"),
    (dict(nside=8, k=8, indices=torch.arange(40, dtype=torch.int32), lut=torch.zeros(768, dtype=torch.int32)), "int64"),
    (dict(nside=8, k=8, indices=torch.arange(40), lut=torch.zeros(767, dtype=torch.int32)), "768"),
    (dict(nside=8, k=8, indices=torch.arange(40), lut=torch.zeros(768, dtype=torch.int64)), "int32"),
    (dict(nside=8, k=8, indices=torch.arange(8), lut=torch.zeros(768, dtype=torch.int32)), "M > k"),
    (dict(nside=8, k=8, indices=torch.arange(40), lut=torch.zeros(768, dtype=torch.int32)), "HIP device"),
    (dict(nside=8, k=8, device="cpu"), "HIP device"),
])
def test_knn_arguments_are_checked_before_the_library(kwargs, match):
    with pytest.raises(ValueError, match=match):
        _native.healpix_knn(**kwargs)


def test_knn_is_declared_in_the_binding():
    assert "dsph_healpix_knn" in _native.SIGNATURES and len(_native.SIGNATURES["dsph_healpix_knn"][1]) == 10


def test_index_sets_are_checked():
    with pytest.raises(ValueError, match="sorted"):
        healpix.healpix_laplacian_ell(8, indices=[5, 3, 9], mode="grid", device="cpu")
    with pytest.raises(ValueError, match="outside"):
        healpix.healpix_laplacian_ell(8, indices=[5, 768], mode="grid", device="cpu")
    with pytest.raises(ValueError, match="power of two"):
        healpix.healpix_laplacian_ell(6, mode="grid", device="cpu")
    with pytest.raises(ValueError, match="unknown graph mode"):
        healpix.healpix_graph_device(8, mode="ring", device="cpu")
    with pytest.raises(NotImplementedError):
        healpix.healpix_laplacian_ell(8, n_neighbors=20, mode="grid", device="cpu")


def test_build_argument():
    layers = [HealpyChebyshev(K=3, Fout=4)]
    with pytest.raises(ValueError, match="build"):
        HealpyGCNN(4, np.arange(192), layers, build="gpu")
    with pytest.raises(ValueError, match="build"):
        HealpyGCNN(4, np.arange(192), layers, build=None)
    model = HealpyGCNN(4, np.arange(192), layers)  # the default is the host path
    assert model.build_mode == "host" and model[0].L is not None
    assert HealpyGCNN(4, np.arange(192), layers, build="host").build_mode == "host"
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            HealpyGCNN(4, np.arange(192), layers, build="device")


# ---- the reference helpers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nside,k", [(4, 8), (8, 8), (8, 20), (8, 40)])
def test_brute_force_agrees_with_the_tree_where_nothing_is_tied(nside, k):
    from scipy.spatial import cKDTree

    vec = gb.vectors(nside)
    nbr, d2, nxt = gb.brute_knn(vec, k)
    dist, tree = cKDTree(vec).query(vec, k=k + 1)
    clear = gb.untied_rows(d2, nxt)
    assert clear.sum() > 0.5 * vec.shape[0]
    assert np.array_equal(np.sort(nbr[clear], axis=1), np.sort(tree[clear, 1:], axis=1))
    np.testing.assert_allclose(np.sqrt(d2[clear]), dist[clear, 1:], rtol=1e-13)
    assert gb.selection_errors(vec, nbr, d2) == []
    # the tree's own selection is valid on every row, tied or not
    tsel = tree[:, 1:]
    td2 = ((vec[tsel] - vec[:, None, :]) ** 2).sum(axis=2)
    order = np.lexsort((tsel, td2), axis=1)
    assert gb.selection_errors(vec, np.take_along_axis(tsel, order, axis=1), np.take_along_axis(td2, order, axis=1)) == []
    assert gb.selection_errors_tree(vec, nbr, d2) == []


def test_the_validity_rule_rejects_wrong_selections():
    vec = gb.vectors(4)
    nbr, d2, _ = gb.brute_knn(vec, 8)
    far = nbr.copy()
    from7 = gb.brute_d2(vec, [7])[0]
    from7[7] = 0.0
    far[7, 0] = int(np.argmax(from7))  # the antipode in place of the nearest neighbour
    fd2 = d2.copy()
    fd2[7, 0] = ((vec[far[7, 0]] - vec[7]) ** 2).sum()
    assert any("beyond the k-th" in e for e in gb.selection_errors(vec, far, fd2))
    assert any("nearer than the k-th" in e for e in gb.selection_errors(vec, far, fd2))
    assert gb.selection_errors_tree(vec, far, fd2) != []
    swapped = nbr.copy()
    swapped[3, [0, 7]] = swapped[3, [7, 0]]
    assert any("ascend" in e for e in gb.selection_errors(vec, swapped, np.take_along_axis(gb.brute_d2(vec), swapped, axis=1)))
    assert any("d2 off" in e for e in gb.selection_errors(vec, nbr, d2 * (1 + 1e-9)))
    twice = nbr.copy()
    twice[5, 1] = twice[5, 0]
    assert any("twice" in e for e in gb.selection_errors(vec, twice, d2))


def test_host_formulas_on_the_trees_selection_give_the_hosts_matrix():
    from scipy.spatial import cKDTree

    for nside, ind, k in ((8, None, 8), (8, None, 20), (16, cap16(), 20)):
        vec = gb.vectors(nside, ind)
        dist, tree = cKDTree(vec).query(vec, k=k + 1)
        kw = healpix.kernel_width(nside, k)
        L = gb.host_laplacian_from_selection(tree[:, 1:], dist[:, 1:] ** 2, kw)
        ref = healpix.healpix_laplacian(nside, indices=ind, n_neighbors=k, mode="knn")
        assert np.array_equal(L.indptr, ref.indptr) and np.array_equal(L.indices, ref.indices)
        np.testing.assert_allclose(L.data, ref.data, rtol=1e-13)


# ---- from a selection to the prepared table, on torch CPU tensors ------------------------------------------------------------------
@pytest.fixture
def brute_kernel(monkeypatch):
    """``_native.healpix_knn`` replaced by the brute-force search (every row ok but the ones named in ``flag``)."""
    state = {"flag": ()}

    def knn(nside, k, indices=None, lut=None, device=None, out=None):
        ind = None if indices is None else indices.numpy()
        nbr, d2, _ = gb.brute_knn(gb.vectors(nside, ind), k)
        ok = np.ones(nbr.shape[0], dtype=np.uint8)
        for r in state["flag"]:
            ok[r], nbr[r], d2[r] = 0, -1, np.nan
        return torch.as_tensor(nbr.astype(np.int32)), torch.as_tensor(d2), torch.as_tensor(ok)

    monkeypatch.setattr(_native, "healpix_knn", knn)
    return state


@pytest.mark.parametrize("nside,full,k", [(4, True, 8), (8, True, 20), (16, False, 20), (16, False, 60)])
def test_assembly_from_a_selection(brute_kernel, nside, full, k):
    ind = None if full else cap16()
    brute_kernel["flag"] = (0, 17, 100)  # these rows come back from the host's tree
    nbr, d2, completed = healpix.healpix_knn_device(nside, ind, k, device="cpu")
    assert completed == 3
    vec = gb.vectors(nside, ind)
    assert gb.selection_errors(vec, nbr.numpy(), d2.numpy()) == []  # (the completed rows included)
    kw = healpix.kernel_width(nside, k)
    g = healpix.healpix_graph_device(nside, ind, k, "knn", device="cpu")
    W = gb.host_graph_from_selection(nbr.numpy(), d2.numpy(), kw)
    assert g.completed == 3 and g.nnz == W.nnz
    cols, vals = g.laplacian_ell()
    L = healpix._normalized_laplacian(W)
    rc, _ = utils.csr_to_ell(L)
    assert cols.dtype == torch.int32 and vals.dtype == torch.float64
    assert np.array_equal(cols.numpy(), rc)
    ref64 = np.zeros(rc.shape)
    lens = np.diff(L.indptr)
    ref64[np.repeat(np.arange(L.shape[0]), lens), np.arange(L.nnz) - np.repeat(L.indptr[:-1], lens)] = L.data
    np.testing.assert_allclose(vals.numpy(), ref64, rtol=0, atol=1e-12)
    assert not np.any(np.signbit(vals.numpy()[ref64 == 0]))  # padding is +0, as the host's
    lens_t = (vals != 0).sum(dim=1)
    assert int(lens_t.min()) >= k + 1 and int(lens_t.max()) <= 2 * k + 1
    nbr_t, nbrT = healpix.healpix_adjacency_tables(nside, ind, k, "knn", device="cpu")
    assert nbrT is nbr_t and np.array_equal(nbr_t.numpy(), utils.adjacency_to_ell(W))


@pytest.mark.parametrize("full", (True, False), ids=("full", "cap"))
def test_grid_tables_equal_the_hosts(full):
    nside, ind = (8, None) if full else (16, cap16())
    cols, vals = healpix.healpix_laplacian_ell(nside, ind, mode="grid", device="cpu")
    L = healpix.healpix_laplacian(nside, indices=ind, mode="grid")
    rc, _ = utils.csr_to_ell(L)
    assert np.array_equal(cols.numpy(), rc)
    lens = np.diff(L.indptr)
    ref64 = np.zeros(rc.shape)
    ref64[np.repeat(np.arange(L.shape[0]), lens), np.arange(L.nnz) - np.repeat(L.indptr[:-1], lens)] = L.data
    np.testing.assert_allclose(vals.numpy(), ref64, rtol=0, atol=1e-12)
    g = healpix.healpix_graph_device(nside, ind, 8, "grid", device="cpu")
    assert np.array_equal(g.adjacency_table().numpy(), utils.adjacency_to_ell(healpix.healpix_graph(nside, ind, 8, "grid")))
    gc, gv = g.laplacian_ell()  # the generic path serves the full sky as well
    assert np.array_equal(gc.numpy(), rc)
    np.testing.assert_allclose(gv.numpy(), ref64, rtol=0, atol=1e-12)


@pytest.mark.parametrize("scale", (0.75, 1.0))
def test_prepare_ell_with_a_given_lmax_is_prepare_L(scale):
    ind = cap16()
    L = healpix.healpix_laplacian(16, indices=ind, mode="grid")
    Lt, lmax = utils.prepare_L(L, scale=scale)
    rc, rv = utils.csr_to_ell(Lt)
    cols, vals = healpix.healpix_laplacian_ell(16, ind, mode="grid", device="cpu")
    pc, pv, plmax = utils.prepare_ell(cols, vals, scale, lmax=lmax)
    assert plmax == lmax and pc is cols
    assert pv.dtype == torch.float32
    pv = pv.numpy()
    assert np.array_equal(pc.numpy(), rc)
    # float64 values 1e-16 apart round to the same float32 but for a handful in 1e9: equal here, and never further than an ulp
    np.testing.assert_allclose(pv, rv, rtol=2e-7, atol=0)
    assert np.mean(pv != rv) < 1e-4
    with pytest.raises(ValueError, match="shape"):
        utils.prepare_ell(cols, vals[:, :-1], scale, lmax=lmax)
