"""CPU tests of HealpySmoothing's host side: the kernel table against an all-pairs construction, the constructor's behaviour, the
stored files and the model builder.  Nothing is smoothed without a GPU."""

import numpy as np
import pytest
import torch

import smoothing_ref as ref
from deepsphere import healpix, healpy_layers
from deepsphere.healpy_layers import HealpyChebyshev, HealpySmoothing
from deepsphere.healpy_networks import HealpyGCNN


def _res(nside):
    return np.sqrt(4 * np.pi / (12 * nside * nside))


@pytest.mark.parametrize("nside,indices", [(4, np.arange(192)), (8, healpix.cap_indices(8))], ids=["n4_full", "n8_cap"])
def test_table_against_all_pairs(nside, indices):
    sigma = 1.0 * _res(nside)
    layer = HealpySmoothing(nside, indices, sigma=sigma, arcmin=False)
    theta, W, d_k, kern = ref.brute_table(nside, indices, sigma, 3)
    cols, vals = layer.cols.numpy(), layer.vals.numpy()
    M = len(indices)
    assert layer.max_neighbors == W and layer.n_indices == M
    assert cols.dtype == np.int32 and vals.dtype == np.float32 and cols.shape == vals.shape == (M, W)
    for m in range(M):
        assert len(set(cols[m].tolist())) == W and cols[m].min() >= 0 and cols[m].max() < M
        present = np.zeros(M, dtype=bool)
        present[cols[m]] = True
        # tie-robust membership: HEALPix symmetry puts several pixels at exactly the cut-off distance
        assert present[theta[m] < d_k[m] * (1 - 1e-9)].all()
        assert (theta[m, cols[m]] <= d_k[m] * (1 + 1e-9)).all()
        want = kern[m, cols[m]] / kern[m, cols[m]].sum()
        np.testing.assert_allclose(vals[m], want, rtol=1e-6, atol=0)
    assert np.abs(vals.astype(np.float64).sum(axis=1) - 1.0).max() <= W * 2.0**-24


def test_fwhm_sigma_and_angle_conversions():
    idx = np.arange(192)
    a = HealpySmoothing(4, idx, fwhm=600.0)
    assert a.sigma_arcmin == pytest.approx(600.0 / np.sqrt(8 * np.log(2))) and a.fwhm_arcmin == pytest.approx(600.0)
    assert a.sigma_rad == pytest.approx(a.sigma_arcmin * np.pi / (60 * 180))
    b = HealpySmoothing(4, idx, sigma=0.1, arcmin=False)
    assert b.sigma_rad == 0.1 and b.sigma_arcmin == pytest.approx(0.1 / np.pi * 180 * 60)
    assert b.fwhm_arcmin == pytest.approx(b.sigma_arcmin * np.sqrt(8 * np.log(2)))
    assert a.do_smoothing and b.do_smoothing and a.n_indices == 192
    assert a.file_label == f"-nside4-sigma{a.sigma_arcmin:4.2f}-n_sigma3"
    assert a.per_channel_repetitions is None


def test_list_scales_become_repetitions():
    idx = np.arange(192)
    s = 0.25  # (a power of two: the ratios are exact, and ceil sees 9, not 9 + 2e-15)
    a = HealpySmoothing(4, idx, sigma=[s, 2 * s, 3 * s], arcmin=False)
    assert a.per_channel_repetitions.tolist() == [1, 4, 9] and a.sigma_rad == pytest.approx(s)
    b = HealpySmoothing(4, idx, fwhm=[3 * 600.0, 600.0, 2 * 600.0])
    assert b.per_channel_repetitions.tolist() == [9, 1, 4] and b.fwhm_arcmin == pytest.approx(600.0)
    c = HealpySmoothing(4, idx, sigma=s, arcmin=False, per_channel_repetitions=[0, 2])
    assert isinstance(c.per_channel_repetitions, np.ndarray) and c.per_channel_repetitions.tolist() == [0, 2]


def test_constructor_assertions():
    idx = np.arange(192)
    with pytest.raises(AssertionError, match="One of fwhm and sigma"):
        HealpySmoothing(4, idx)
    with pytest.raises(AssertionError, match="Only one of fwhm and sigma"):
        HealpySmoothing(4, idx, fwhm=600.0, sigma=300.0)
    with pytest.raises(AssertionError, match="per_channel_repetitions can't be specified"):
        HealpySmoothing(4, idx, sigma=[300.0, 600.0], per_channel_repetitions=[1, 2])
    with pytest.raises(AssertionError, match="per_channel_repetitions can't be specified"):
        HealpySmoothing(4, idx, fwhm=[300.0, 600.0], per_channel_repetitions=[1, 2])


def test_zero_scale_is_the_identity_on_a_cpu_tensor():
    x = torch.randn(2, 192, 3)
    for kw in ({"sigma": 0.0}, {"fwhm": 0}):
        layer = HealpySmoothing(4, np.arange(192), **kw)
        assert not layer.do_smoothing
        assert layer(x) is x and layer.call(x) is x


def test_ring_ordering_is_refused():
    with pytest.raises(NotImplementedError, match="only NEST ordering is supported"):
        HealpySmoothing(4, np.arange(192), nest=False, sigma=600.0)


def test_build_checks_the_input_shape():
    layer = HealpySmoothing(4, np.arange(192), sigma=600.0, per_channel_repetitions=[1, 2], max_batch_size=4)
    with pytest.raises(AssertionError):
        layer.build((2, 191, 2))
    with pytest.raises(AssertionError, match="has to have length 3"):
        layer.build((2, 192, 3))
    layer.build((2, 192, 2))
    assert layer.n_channels == 2 and layer.n_batch == 4 and layer.n_matmul_splits == 1
    masked = HealpySmoothing(4, np.arange(192), sigma=600.0, mask=np.ones(191, dtype=bool))
    with pytest.raises(AssertionError, match="The mask has to have shape"):
        masked.build((2, 192, 2))
    for shape in ((192,), (192, 1), (192, 2)):
        ok = HealpySmoothing(4, np.arange(192), sigma=600.0, mask=np.ones(shape, dtype=bool))
        ok.build((2, 192, 2))
        assert tuple(ok.mask.shape) == (1, 192, shape[1] if len(shape) == 2 else 1) and ok.mask.dtype == torch.float32


def test_no_cpu_fallback():
    layer = HealpySmoothing(4, np.arange(192), sigma=600.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer(torch.randn(2, 192, 1))


def test_data_path_stores_and_loads_the_reference_files(tmp_path, monkeypatch):
    idx = healpix.cap_indices(8)
    first = HealpySmoothing(8, idx, sigma=1.0 * _res(8), arcmin=False, data_path=str(tmp_path))
    M, W = first.n_indices, first.max_neighbors
    ind = np.load(tmp_path / f"ind_coo{first.file_label}.npy")
    val = np.load(tmp_path / f"val_coo{first.file_label}.npy")
    assert ind.dtype == np.int64 and ind.shape == (M * W, 2) and val.dtype == np.float32 and val.shape == (M * W,)
    assert np.array_equal(ind[:, 0], np.repeat(np.arange(M), W)) and val.max() == 1.0  # not normalised: the pixel itself

    def refuse(self):
        raise AssertionError("the table was rebuilt although the files exist")

    monkeypatch.setattr(HealpySmoothing, "_build_tree", refuse)
    second = HealpySmoothing(8, idx, sigma=1.0 * _res(8), arcmin=False, data_path=str(tmp_path))
    assert second.max_neighbors == W
    assert torch.equal(first.cols, second.cols) and torch.equal(first.vals, second.vals)
    # the files in another order of entries (the reference sorts what it loads) give the same table
    perm = np.random.default_rng(0).permutation(M * W)
    np.save(tmp_path / f"ind_coo{first.file_label}.npy", ind[perm])
    np.save(tmp_path / f"val_coo{first.file_label}.npy", val[perm])
    third = HealpySmoothing(8, idx, sigma=1.0 * _res(8), arcmin=False, data_path=str(tmp_path))
    assert torch.equal(first.cols, third.cols) and torch.equal(first.vals, third.vals)
    with pytest.raises(AssertionError, match="rebuilt"):
        HealpySmoothing(8, idx, sigma=2.0 * _res(8), arcmin=False, data_path=str(tmp_path))  # another label: no file


def test_transposed_table_is_lazy_and_padded_in_bounds():
    layer = HealpySmoothing(8, healpix.cap_indices(8), sigma=1.0 * _res(8), arcmin=False)
    assert layer._tables_T is None
    colsT, valsT = layer._transposed_tables(torch.device("cpu"))
    M = layer.n_indices
    assert colsT.dtype == torch.int32 and valsT.dtype == torch.float32 and colsT.shape == valsT.shape and colsT.shape[0] == M
    assert int(colsT.min()) >= 0 and int(colsT.max()) < M
    K = ref.dense(layer.cols.numpy(), layer.vals.numpy())
    assert np.array_equal(ref.dense(colsT.numpy(), valsT.numpy()), K.T)
    pad = valsT.numpy() == 0
    assert pad.any() and np.array_equal(colsT.numpy()[pad], np.nonzero(pad)[0])
    assert colsT.shape[1] == int((K != 0).sum(axis=0).max())


def test_in_a_healpy_gcnn():
    idx = healpix.cap_indices(8)
    smooth = HealpySmoothing(8, idx, sigma=1.0 * _res(8), arcmin=False)
    model = HealpyGCNN(8, idx, [smooth, HealpyChebyshev(K=3, Fout=4, device="cpu")])
    assert model[0] is smooth and np.array_equal(model.indices_out, idx) and model.nside_out == 8
    assert "HealpySmoothing" in healpy_layers.__all__


def test_single_pass_helper_against_the_dense_matrix_with_empty_slots():
    """``smoothing_ref.apply_pass`` (the reference of the GPU tests on synthetic tables) against ``dense()``: entries outside
    [0, M) carry weight 0 wherever they stand in a row, a row of nothing else gives 0, and ``reps`` / ``pass_index`` / mask select
    and scale as ``_native.ell_smooth`` documents."""
    rng = np.random.default_rng(0)
    M, W, C = 37, 49, 4
    cols = rng.integers(0, M, size=(M, W)).astype(np.int32)
    vals = rng.random((M, W)).astype(np.float32)
    bad = rng.random((M, W)) < 1 / 3
    bad[11] = True                                                   # a row without a valid entry
    cols[bad] = rng.choice(np.array([-1, M, M + 5, 2**31 - 1], dtype=np.int32), size=int(bad.sum()))
    assert bad[:, 0].any() and bad[:, W // 2].any() and not bad[:, -1].all()  # anywhere in the row, not only at its end
    x = rng.standard_normal((2, M, C))
    K = ref.dense(np.where(bad, 0, cols), np.where(bad, 0.0, vals))  # the valid entries alone
    want = np.einsum("mk,nkc->nmc", K, x)
    got = ref.apply_pass(cols, vals, x)
    assert np.abs(got - want).max() <= 1e-12 * W and (got[:, 11] == 0).all()
    # the raw-column helper is a different function on such a table (a -1 wraps to the last pixel)
    wrapped = np.where(cols == -1, cols, np.where(bad, 0, cols))
    assert np.abs(ref.apply(wrapped, np.where(bad & (cols != -1), 0.0, vals), x) - want).max() > 1e-3
    # on a table without empty slots the two helpers agree
    clean = rng.integers(0, M, size=(M, W)).astype(np.int32)
    assert np.array_equal(ref.apply_pass(clean, vals, x), ref.apply(clean, vals, x))
    # reps, pass_index and masks
    reps = [0, 1, 3, 2]
    for mask in (rng.random((M, 1)), rng.random((M, C))):
        for pass_index in range(3):
            out = ref.apply_pass(cols, vals, x, reps, pass_index, mask)
            for c in range(C):
                src = want if reps[c] > pass_index else x
                assert np.abs(out[:, :, c] - src[:, :, c] * mask[None, :, c % mask.shape[1]]).max() <= 1e-12 * W
