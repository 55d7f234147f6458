"""CPU tests of the graph transformer's host side: the neighbour tables, constructor checks, the spec and the model builder.
No attention is computed without a GPU."""

import numpy as np
import pytest
import torch
from scipy import sparse

import deepsphere
from deepsphere import _native, gnn_transformers, healpix, healpy_layers, utils
from deepsphere.healpy_layers import Healpy_Transformer, HealpyPool


def _check_table(A, nbr):
    """The table lists exactly the positions A.nonzero() reports, row by row, ascending, then -1."""
    A = sparse.csr_matrix(A)
    M = A.shape[0]
    rows, cols = A.nonzero()
    assert nbr.dtype == np.int32 and nbr.shape[0] == M
    lens = np.bincount(rows, minlength=M)
    assert nbr.shape[1] == max(int(lens.max()), 1)
    for i in range(M):
        want = np.sort(cols[rows == i])
        assert np.array_equal(nbr[i, :lens[i]], want)
        assert np.all(nbr[i, lens[i]:] == -1)
    return lens


def test_adjacency_to_ell_on_healpix_graphs():
    lens = _check_table(healpix.healpix_graph(4), utils.adjacency_to_ell(healpix.healpix_graph(4)))
    assert lens.min() == 8 and lens.max() == 9
    A = healpix.healpix_graph(4, mode="grid")
    nbr = utils.adjacency_to_ell(A)
    lens = _check_table(A, nbr)
    assert lens.min() == 7 and lens.max() == 8 and (nbr == -1).any()  # the 24 corner pixels: padding appears


def _small_asymmetric():
    # 5 nodes; (0, 3) is stored with value 0 -- not an edge; row 2 is empty
    rows = np.array([0, 0, 0, 1, 3, 3, 4])
    cols = np.array([4, 1, 3, 0, 2, 0, 4])
    vals = np.array([1.0, 2.0, 0.0, 1.0, 3.0, 1.0, 1.0])
    return sparse.csr_matrix((vals, (rows, cols)), shape=(5, 5))


def test_adjacency_to_ell_asymmetric_stored_zero_and_empty_row():
    A = _small_asymmetric()
    assert A.nnz == 7  # the zero is stored
    nbr = utils.adjacency_to_ell(A)
    assert nbr.tolist() == [[1, 4], [0, -1], [-1, -1], [0, 2], [4, -1]]
    _check_table(A, nbr)
    # a matrix without any edge still has one (unused) slot
    assert utils.adjacency_to_ell(sparse.csr_matrix((3, 3))).tolist() == [[-1], [-1], [-1]]
    with pytest.raises(ValueError):
        utils.adjacency_to_ell(sparse.csr_matrix((3, 4)))


def test_transposed_table_is_the_table_of_the_transpose():
    A = _small_asymmetric()
    nbr, nbrT = gnn_transformers.neighbour_tables(A)
    assert nbr is not nbrT
    assert np.array_equal(nbrT.numpy(), utils.adjacency_to_ell(A.T))
    assert nbrT.tolist() == [[1, 3], [0, -1], [3, -1], [-1, -1], [0, 4]]
    # in-edges of the table are the out-edges of the transposed one
    e = {(i, int(j)) for i in range(5) for j in nbr[i].tolist() if j >= 0}
    eT = {(int(i), j) for j in range(5) for i in nbrT[j].tolist() if i >= 0}
    assert e == eT
    # a symmetric graph shares ONE tensor
    s, sT = gnn_transformers.neighbour_tables(healpix.healpix_graph(4))
    assert s is sT


def test_constructor_checks():
    A = healpix.healpix_graph(2)
    with pytest.raises(ValueError):
        gnn_transformers.MultiHeadAttention(d_model=10, num_heads=4)
    with pytest.raises((ValueError, AssertionError)):
        gnn_transformers.Graph_Transformer(A, key_dim=4, num_heads=2, n_layers=0)
    with pytest.raises(ValueError):
        gnn_transformers.MultiHeadAttention(d_model=8, num_heads=2, activation="no_such_activation")
    layer = gnn_transformers.Graph_Transformer(A, key_dim=4, num_heads=2, n_layers=2)
    assert layer.Fout == layer.embedding_size == 8 and len(layer.mha_layers) == 2
    names = {n for n, _ in layer.named_parameters()}
    for i in range(2):
        for leaf in ("wqkv.weight", "wqkv.bias", "dense.weight", "dense.bias", "layer_norm1.weight", "layer_norm2.bias"):
            assert f"mha_layers.{i}.{leaf}" in names
    m = layer.mha_layers[0]
    assert tuple(m.wqkv.weight.shape) == (24, 8) and float(m.wqkv.bias.detach().abs().max()) == 0.0
    assert float(m.wqkv.weight.detach().abs().max()) <= np.sqrt(6.0 / 16.0)  # every block Glorot-uniform with the fans of ONE Dense(d)
    assert m.layer_norm1.eps == 1e-3
    # identity norms, documented: the reference crashes with use_norm=False
    m = gnn_transformers.MultiHeadAttention(8, 2, use_norm=False)
    assert isinstance(m.layer_norm1, torch.nn.Identity) and isinstance(m.layer_norm2, torch.nn.Identity)
    # the position embedding: (1, M, d), Glorot-uniform with Keras' fans for that shape
    pe = gnn_transformers.AddPositionEmbs()
    pe.build((1, 48, 8))
    assert tuple(pe.pos_embedding.shape) == (1, 48, 8) and float(pe.pos_embedding.detach().abs().max()) <= np.sqrt(6.0 / 56.0)


def test_dense_attention_is_not_built_and_cpu_inputs_raise():
    m = gnn_transformers.MultiHeadAttention(8, 2)
    with pytest.raises(NotImplementedError, match="ViT"):
        m(torch.zeros(1, 48, 8))
    if not torch.cuda.is_available():
        layer = gnn_transformers.Graph_Transformer(healpix.healpix_graph(2), key_dim=4, num_heads=2)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            layer(torch.zeros(1, 48, 3))
        t = torch.zeros(1, 48, 8)
        nbr, nbrT = gnn_transformers.neighbour_tables(healpix.healpix_graph(2))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            gnn_transformers.scaled_dot_product_sparse_attention(t, t, t, nbr, nbrT, 2)


def test_c_abi_names_the_limit_it_refuses():
    """Shapes outside the kernel's return -1 with the limit in the message before anything touches a device."""
    import ctypes

    lib = _native.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    p = ctypes.c_void_p((p.value + 15) & ~15)

    def fwd(ld=8, width=1, heads=2, depth=4, q=p):
        return lib.dsph_nbr_attention_forward(q, p, p, ld, p, None, p, width, 1, 1, heads, depth, 0, None)

    assert fwd(depth=5) == -1 and "4, 8, 16, 32, 64" in _native.last_error()
    assert fwd(heads=5, depth=64, ld=320) == -1 and "256" in _native.last_error()
    assert fwd(heads=0) == -1
    assert fwd(width=0) == -1 and "width" in _native.last_error()
    assert fwd(ld=10) == -1 and "multiple of 4" in _native.last_error()
    assert fwd(ld=4) == -1 and "stride" in _native.last_error()
    assert fwd(q=ctypes.c_void_p(p.value + 4)) == -1 and "16-byte" in _native.last_error()
    assert fwd(q=None) == -1 and "NULL" in _native.last_error()
    rc = lib.dsph_nbr_attention_backward(p, p, p, 8, p, p, p, p, 1, p, 0, p, p, p, p, 8, 1, 1, 2, 4, 0, None)
    assert rc == -1 and "width" in _native.last_error()


def test_healpy_transformer_spec_round_trip():
    spec = Healpy_Transformer(key_dim=8, num_heads=2, positional_encoding=False, n_layers=3, activation="elu", layer_norm=False)
    assert (spec.key_dim, spec.num_heads, spec.positional_encoding, spec.n_layers, spec.activation, spec.layer_norm) == (
        8, 2, False, 3, "elu", False)
    A = healpix.healpix_graph(2)
    layer = spec._get_layer(A)
    assert isinstance(layer, gnn_transformers.Graph_Transformer)
    assert (layer.key_dim, layer.num_heads, layer.positional_encoding, layer.n_layers, layer.activation, layer.layer_norm) == (
        8, 2, False, 3, "elu", False)
    assert layer.A is A and layer.Fout == 16 and len(layer.mha_layers) == 3 and not hasattr(layer, "pos_encoder")
    assert "Healpy_Transformer" in healpy_layers.__all__ and deepsphere.Healpy_Transformer is Healpy_Transformer
    assert deepsphere.Graph_Transformer is gnn_transformers.Graph_Transformer


def test_healpy_gcnn_builds_graph_transformers():
    model = deepsphere.HealpyGCNN(8, np.arange(768), [Healpy_Transformer(8, 2), HealpyPool(1), Healpy_Transformer(8, 2)])
    gts = [m for m in model if isinstance(m, gnn_transformers.Graph_Transformer)]
    assert len(gts) == 2 and len(model) == 3
    assert gts[0].nbr.shape[0] == 768 and gts[1].nbr.shape[0] == 192
    assert gts[0].nbrT is gts[0].nbr  # HEALPix graphs are symmetric
    assert np.array_equal(gts[1].nbr.numpy(), utils.adjacency_to_ell(healpix.healpix_graph(4)))
    # the 20-neighbour graph and the grid stencil reach the layer too
    model = deepsphere.HealpyGCNN(4, np.arange(192), [Healpy_Transformer(4, 1)], n_neighbors=20)
    assert 20 <= model[0].nbr.shape[1] <= 22
    model = deepsphere.HealpyGCNN(4, np.arange(192), [Healpy_Transformer(4, 1)], graph_mode="grid")
    assert model[0].nbr.shape[1] == 8
