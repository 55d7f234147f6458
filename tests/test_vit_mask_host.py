"""CPU tests of the dense attention's ``mask`` argument: ``healpix.superpixel_padding_mask``, the layout and the refusals of the
mask operand (``_native.attention_mask``), the two ``_masked`` entry points of the C ABI (exports, named argument errors), the
layers' rules (a mask with neighbour tables, a mask that requires grad, constructor and call precedence) and the helper of the
GPU tests (tests/dense_attention_mask_ref.py) against float64 autograd.  No attention is computed without a GPU."""

import ctypes

import numpy as np
import pytest
import torch
from scipy import sparse

import dense_attention_mask_ref as mref
import dense_attention_ref as ref
from deepsphere import _native, gnn_transformers, healpix
from deepsphere.healpy_layers import Healpy_ViT
from helpers import rel_err

BADARG, UNSUPPORTED = -1, -3


# ---- healpix.superpixel_padding_mask

def test_a_full_footprint_masks_nothing():
    idx = np.arange(768)
    for p in (1, 2):
        mask = healpix.superpixel_padding_mask(idx, idx, p)
        assert mask.dtype == np.float32 and mask.shape == (768 // 4 ** p,) and not mask.any()


def test_whole_missing_superpixels_are_marked_and_partly_filled_ones_are_not():
    nside, p = 8, 1
    footprint = healpix.cap_indices(nside, fraction=0.2)
    idx = healpix.extend_indices(footprint, nside, nside // 2)
    free = np.setdiff1d(np.arange(192), idx // 4)[[0, -1]]  # two parents the footprint does not touch: padding only
    extra = (4 * free[:, None] + np.arange(4)).reshape(-1)
    idx = np.union1d(idx, extra)
    mask = healpix.superpixel_padding_mask(idx, footprint, p)
    parents = np.unique(idx // 4)
    assert mask.shape == (idx.size // 4,) and mask.dtype == np.float32
    assert set(parents[mask == 1.0]) == set(free)  # exactly the super-pixels without a footprint pixel, in the coarsened order
    partly = [par for par in parents if 0 < np.isin(4 * par + np.arange(4), footprint).sum() < 4]
    assert partly, "the cap's rim must cut some super-pixels for this test to mean anything"
    assert not mask[np.isin(parents, partly)].any()  # one data pixel keeps a super-pixel attended
    # p = 2 on a set closed under two coarsenings; the footprint's order and duplicates do not matter
    free2 = np.setdiff1d(np.arange(48), footprint // 16)[0]
    idx2 = healpix.extend_indices(np.union1d(footprint, [16 * free2 + 7]), nside, nside // 4)
    mask2 = healpix.superpixel_padding_mask(idx2, np.concatenate([footprint[::-1], footprint[:5]]), 2)
    assert mask2.shape == (idx2.size // 16,)
    assert set(np.unique(idx2 // 16)[mask2 == 1.0]) == {free2}


def test_indices_not_closed_under_p_raise():
    idx = np.arange(768)
    with pytest.raises(ValueError, match="closed under p = 1"):
        healpix.superpixel_padding_mask(idx[1:-3], idx, 1)  # a multiple of 4 ids, parents without all children
    with pytest.raises(ValueError, match="closed under p = 1"):
        healpix.superpixel_padding_mask(idx[:-1], idx, 1)
    with pytest.raises(ValueError, match="closed under p = 2"):
        healpix.superpixel_padding_mask(healpix.extend_indices([5, 700], 8, 4), idx, 2)  # closed under one coarsening only
    with pytest.raises(ValueError, match="sorted"):
        healpix.superpixel_padding_mask(idx[::-1], idx, 1)
    with pytest.raises(ValueError, match="at least 1"):
        healpix.superpixel_padding_mask(idx, idx, 0)


# ---- the mask operand

N, HEADS, M = 3, 2, 5


@pytest.mark.parametrize("shape,strides", [((M,), (0, 0, 0)), ((N, 1, 1, M), (M, 0, 0)), ((1, HEADS, 1, M), (0, M, 0)),
                                           ((M, M), (0, 0, M)), ((N, HEADS, M, M), (HEADS * M * M, M * M, M)),
                                           ((N, 1, M, M), (M * M, 0, M)), ((HEADS, 1, M), (0, M, 0))])
def test_every_broadcast_form_is_one_operand(shape, strides):
    mask = torch.arange(int(np.prod(shape)), dtype=torch.float32).reshape(shape)
    t, got = _native.attention_mask(mask, N, HEADS, M)
    assert got == strides and t.dim() == 4 and t.shape[3] == M and t.stride(3) == 1 and t.dtype == torch.float32
    assert t.data_ptr() == mask.data_ptr()  # nothing was copied, nothing of size N heads M M allocated for a broadcast mask
    assert t.numel() == mask.numel()
    full = mask.reshape((1,) * (4 - mask.dim()) + tuple(shape)).expand(N, HEADS, M, M)
    flat = mask.flatten()  # (the operand starts where the mask starts: the kernels' address arithmetic on it)
    for n, h, i, j in ((0, 0, 0, 0), (2, 1, 3, 4), (1, 0, 4, 2)):
        assert flat[n * got[0] + h * got[1] + i * got[2] + j] == full[n, h, i, j]


def test_mask_conversions():
    t, s = _native.attention_mask(np.array([True, False, True, False, False]), N, HEADS, M)  # bool -> float32
    assert t.dtype == torch.float32 and t.flatten().tolist() == [1, 0, 1, 0, 0] and s == (0, 0, 0)
    t, s = _native.attention_mask(torch.tensor([[1], [0], [2]], dtype=torch.int64).reshape(N, 1, 1, 1), N, HEADS, M)  # int, last dim 1
    assert t.dtype == torch.float32 and tuple(t.shape) == (N, 1, 1, M) and s == (M, 0, 0) and t[2, 0, 0].tolist() == [2.0] * M
    t, s = _native.attention_mask(torch.zeros(M, M, dtype=torch.float64).t(), N, HEADS, M)  # last dimension not contiguous: a copy
    assert t.stride(3) == 1 and s == (0, 0, M)
    wide = torch.zeros(M, M + 3)
    t, s = _native.attention_mask(wide[:, :M], N, HEADS, M)  # a view with longer rows is read in place
    assert t.data_ptr() == wide.data_ptr() and s == (0, 0, M + 3)
    t, s = _native.attention_mask(torch.zeros(1, M).expand(M, M), N, HEADS, M)  # an expanded view keeps its zero stride
    assert s == (0, 0, 0)


@pytest.mark.parametrize("shape", [(M + 1,), (N + 1, 1, 1, M), (1, HEADS + 1, 1, M), (M - 1, M), (M, 2), (1, 1, 1, M, M), (N, HEADS, M, 3)])
def test_a_shape_that_does_not_broadcast_names_both_shapes(shape):
    with pytest.raises(ValueError) as e:
        _native.attention_mask(torch.zeros(shape), N, HEADS, M)
    assert str(tuple(shape)) in str(e.value) and str((N, HEADS, M, M)) in str(e.value)


def test_a_mask_that_requires_grad_raises():
    mask = torch.zeros(M, requires_grad=True)
    with pytest.raises(ValueError, match="not differentiable"):
        _native.attention_mask(mask, N, HEADS, M)
    q = torch.zeros(N, M, 8)
    with pytest.raises(ValueError, match="not differentiable"):  # (before the device is asked for)
        gnn_transformers.scaled_dot_product_attention(q, q, q, HEADS, mask=mask)
    with pytest.raises(ValueError, match="not differentiable"):
        gnn_transformers.MultiHeadAttention(8, HEADS, dense=True)(q, mask=mask)
    with pytest.raises(ValueError, match="not differentiable"):
        Healpy_ViT(1, 4, HEADS, mask=mask)
    _native.attention_mask(mask.detach(), N, HEADS, M)


# ---- the C ABI

def _aligned_buffer():
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    return buf, ctypes.c_void_p((p.value + 15) & ~15)


def test_exports():
    for name in ("dsph_dense_attention_forward_masked", "dsph_dense_attention_backward_masked"):
        assert name in _native.SIGNATURES and hasattr(_native.lib(), name)
    assert _native.lib().dsph_abi_version() == 3


@pytest.mark.parametrize("precision", [_native.PREC_FP32, _native.PREC_BF16X6, _native.PREC_BF16X3])
def test_masked_entry_points_name_what_they_refuse(precision):
    lib = _native.lib()
    buf, p = _aligned_buffer()

    def fwd(ld=64, M=1, heads=2, depth=32, q=p, mask=p, strides=(0, 0, 0), prec=precision, stat=None):
        return lib.dsph_dense_attention_forward_masked(q, p, p, ld, p, stat, mask, *strides, 1, M, heads, depth, prec, 0, None)

    def bwd(ld=64, ld_grad=64, M=1, heads=2, depth=32, q=p, mask=p, strides=(0, 0, 0), prec=precision, stat=p):
        return lib.dsph_dense_attention_backward_masked(q, p, p, ld, p, stat, mask, *strides, p, p, p, p, p, ld_grad, 1, M, heads, depth,
                                                        prec, 0, None)

    for call in (fwd, bwd):
        assert call(mask=None) == BADARG and "NULL mask" in _native.last_error()
        for strides in ((-1, 0, 0), (0, -8, 0), (0, 0, -1)):
            assert call(strides=strides) == BADARG and "negative mask stride" in _native.last_error()
        assert call(q=None) == BADARG and "NULL" in _native.last_error()
        assert call(depth=5, ld=12) == BADARG and "4, 8, 16, 32, 64" in _native.last_error()
        assert call(ld=66) == BADARG and "multiple of 4" in _native.last_error()
        assert call(M=0) == BADARG and "at least 1" in _native.last_error()
        assert call(q=ctypes.c_void_p(p.value + 4)) == BADARG and "16-byte" in _native.last_error()
        assert call(stat=ctypes.c_void_p(p.value + 4)) == BADARG and "8-byte" in _native.last_error()
        assert call(prec=99) == BADARG and "precision" in _native.last_error()
        if precision != _native.PREC_FP32:
            assert call(depth=16, ld=32) == UNSUPPORTED and "32, 64" in _native.last_error()
    assert bwd(stat=None) == BADARG and "NULL" in _native.last_error()
    assert bwd(ld_grad=66) == BADARG and "gradients" in _native.last_error()


# ---- the layers

def test_a_mask_with_neighbour_tables_raises():
    x = torch.zeros(2, 48, 8)
    mask = torch.zeros(48)
    A = sparse.csr_matrix(np.roll(np.eye(48), 1, axis=1) + np.roll(np.eye(48), -1, axis=1))  # a ring
    block = gnn_transformers.MultiHeadAttention(8, 2, sparse_A_indices=A)
    with pytest.raises(ValueError, match="takes no mask"):  # the reference would drop it silently
        block(x, mask=mask)
    with pytest.raises(ValueError, match="takes no mask"):
        gnn_transformers.MultiHeadAttention(8, 2)(x, gnn_transformers.neighbour_tables(A), mask=mask)
    with pytest.raises(TypeError):
        gnn_transformers.Graph_Transformer(A, 4, 2)(x, mask=mask)  # no mask argument on the neighbour-attention layers


def test_constructor_mask_is_a_non_persistent_buffer():
    mask = np.array([1, 0, 0, 1, 0], dtype=bool)
    layer = Healpy_ViT(1, 4, 2, n_layers=2, mask=mask)
    assert isinstance(layer.mask, torch.Tensor) and layer.mask.dtype == torch.float32 and layer.mask.tolist() == [1, 0, 0, 1, 0]
    assert "mask" in dict(layer.named_buffers()) and "mask" not in layer.state_dict()
    assert layer.to(torch.float32).mask is not None
    plain = gnn_transformers.Graph_ViT(1, 4, 2)
    assert plain.mask is None and not dict(plain.named_buffers())
    old = gnn_transformers.Graph_ViT(1, 4, 2, True, 1, "relu", True, "fp32")  # the positional arguments before `mask` are unchanged
    assert old.mask is None
    with pytest.raises(ValueError, match="does not broadcast"):
        gnn_transformers.Graph_ViT(1, 4, 2, mask=np.zeros((1, 1, 1, 1, 5)))


def test_the_call_mask_takes_precedence_over_the_constructor_mask(monkeypatch):
    """Graph_ViT.forward without a device: the embedding runs in torch; the blocks are replaced by recorders of the mask they get."""
    seen = []

    class Recorder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.wqkv = torch.nn.Linear(1, 1)

        def forward(self, x, tables=None, mask=None):
            seen.append(mask)
            return x

    monkeypatch.setattr(gnn_transformers, "_require_hip", lambda *t: None)
    ctor, call = torch.tensor([1.0, 0, 0, 0, 0, 0]), torch.tensor([0.0, 0, 1, 1, 0, 0])
    layer = gnn_transformers.Graph_ViT(1, 4, 2, n_layers=2, mask=ctor)
    layer.mha_layers = torch.nn.ModuleList([Recorder(), Recorder()])
    x = torch.zeros(2, 24, 3)
    layer(x)
    assert len(seen) == 2 and all(tuple(m.shape) == (1, 1, 1, 6) and m.flatten().tolist() == ctor.tolist() for m in seen)
    assert seen[0] is seen[1]  # laid out once, the same operand to every block
    del seen[:]
    layer(x, mask=call)
    assert all(m.flatten().tolist() == call.tolist() for m in seen) and len(seen) == 2
    del seen[:]
    layer(x, mask=np.zeros((2, 1, 6, 6), dtype=np.int32))
    assert all(tuple(m.shape) == (2, 1, 6, 6) and m.dtype == torch.float32 for m in seen)
    with pytest.raises(ValueError) as e:
        layer(x, mask=torch.zeros(24))  # a mask over the pixels, not over the 6 super-pixels
    assert "(24,)" in str(e.value) and "(2, 2, 6, 6)" in str(e.value)
    del seen[:]
    plain = gnn_transformers.Graph_ViT(1, 4, 2)
    plain.mha_layers = torch.nn.ModuleList([Recorder()])
    plain(x)
    assert seen == [None]


# ---- the helper of the GPU tests

def _case(M=37, heads=2, depth=8, seed=0):
    rng = np.random.default_rng(seed)
    q, k, v, g = (rng.standard_normal((2, M, heads * depth)).astype(np.float32) for _ in range(4))
    mask = (rng.uniform(size=(2, 1, M, M)) < 0.3).astype(np.float32)
    mask[:, :, :, 0] = 0
    return q, k, v, g, mask


def test_helper_gradients_are_those_of_float64_autograd():
    q, k, v, g, mask = _case()
    out, stat, dq, dk, dv = mref.attention(q, k, v, 2, mask, g)
    t = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (q, k, v)]
    want = mref.attention_torch(t[0], t[1], t[2], 2, mask)
    want.backward(torch.tensor(g, dtype=torch.float64))
    for got, w in zip((out, dq, dk, dv), (want.detach(), t[0].grad, t[1].grad, t[2].grad)):
        assert rel_err(got, w.numpy()) < 1e-6  # (the helper rounds the logits to float32; autograd does not)
    # zero mask: the unmasked reference, and lse = m + log l
    zero = mref.attention(q, k, v, 2, np.zeros(37, dtype=np.float32))
    want_out, _, want_lse = ref.attention_np(q, k, v, 2)
    assert rel_err(zero[0], want_out) < 1e-6 and rel_err(zero[1].sum(-1), want_lse) < 1e-6


def test_helper_fully_masked_row_and_soft_bias():
    q, k, v, g, mask = _case()
    mask[:, :, 5, :] = 1
    out, stat, dq, dk, dv = mref.attention(q, k, v, 2, mask, g)
    assert np.isfinite(out).all() and all(np.isfinite(a).all() for a in (dq, dk, dv))
    assert rel_err(out[:, 5], v.astype(np.float64).mean(axis=1)) < 1e-12  # uniform softmax: the mean of v
    assert (stat[:, 5, :, 0] == -1e9).all() and np.allclose(stat[:, 5, :, 1], np.log(37))
    # 2.5e-9 on one key lowers its logit by 2.5: the same as scaling that key's probability by exp(-2.5) before normalising
    soft = np.zeros(37, dtype=np.float32)
    soft[3] = 2.5e-9
    a = mref.attention(q, k, v, 2, soft)[1]
    b = mref.attention(q, k, v, 2, np.zeros(37, dtype=np.float32))[1]
    assert not np.array_equal(a, b) and np.abs(a.sum(-1) - b.sum(-1)).max() < 2.5
    with pytest.raises(AssertionError):
        mref.attention(20 * q, 20 * k, v, 2, soft)  # logits past the helper's limit


def test_split_emulation_with_a_mask_is_close_to_the_reference():
    q, k, v, g, mask = _case(M=40, heads=1, depth=32)
    want = mref.attention(q, k, v, 1, mask, g)
    for precision, bound in (("bf16x6", 1e-6), ("bf16x3", 1e-4)):
        got = mref.split_attention(q, k, v, 1, precision, mask, g)
        errs = [rel_err(a, b) for a, b in zip(got, want)]
        assert max(errs) < bound, (precision, errs)
    assert max(rel_err(a, b) for a, b in zip(mref.split_attention(q, k, v, 1, "bf16x3", mask, g), want)) > 1e-7
