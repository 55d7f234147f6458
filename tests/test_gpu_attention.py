"""GPU tests of the neighbour-attention kernels and the graph transformer built on them (``pytest -m gpu``).

Reference: tests/attention_ref.py, the reference's edge-list algorithm restated in float64.  Error measure: helpers.rel_err
(max |a - b| / max |b|).  Tolerances: 1e-5 forward and 2e-5 gradients, the project's fp32 tolerances (torch fp32 on the CPU
sits at 2e-7 on these inputs); 1e-4 for the large-logit case, where the rounding of a logit of size 150 alone is
150 * 2^-23 * a few = 5e-5 (torch fp32 on the CPU: 1.7e-6); the whole layer, whose GEMMs and norms are the library's, ten times
the error the same layer shows in torch fp32 on the CPU, computed in the test.  N = 2 throughout.

Lane layouts.  A row takes lpr = d / 4 lanes and a wave rpw = floor(64 / lpr) rows; a head takes LPH = depth / 4 lanes, summed
by log2(LPH) xor shuffles.  The cases visit every instantiated depth, forward and backward (LPH 1, 2, 4, 8, 16: the shuffle loop
has zero to four trips), and with them lpr in {1, 2, 5, 6, 12, 16, 32, 64}: rows that divide the wave (1, 2, 16, 32, 64), rows that
leave idle lanes (5 -> 12 rows and 4 idle lanes, 6 -> 10 rows and 4 idle lanes, 12 -> 5 rows and 4 idle lanes), and d = 256 both
as 8 heads of 32 and as 64 heads of 4 (a head per lane).
"""

import functools

import numpy as np
import pytest
import torch

import attention_ref as ref
import deepsphere
from deepsphere import _native, gnn_transformers, healpix
from deepsphere.healpy_layers import Healpy_Transformer, HealpyChebyshev, HealpyPool
from helpers import offset_view, padded_view, rel_err

pytestmark = pytest.mark.gpu

N = 2
SHAPES = [(1, 4), (4, 16), (2, 64), (3, 16), (4, 64)]  # (3, 16): 12 lanes per row, idle lanes; (4, 64): one row per wave
# the depths 8 and 32, and depth 4 past one lane per row: (heads, depth) -> lanes per row, rows per wave
OTHER_DEPTHS = {(1, 8): (2, 32), (3, 8): (6, 10), (2, 32): (16, 4), (8, 32): (64, 1), (5, 4): (5, 12), (64, 4): (64, 1)}
BACKWARD_OTHER_DEPTHS = [(1, 4), (5, 4), (3, 8), (2, 32), (8, 32)]


@functools.lru_cache(maxsize=None)
def graph(name):
    """-> (A, rows, cols, nbr, nbrT) with the tables on the GPU."""
    if name == "n4_knn":
        A = healpix.healpix_graph(4)
    elif name == "n4_grid":
        A = healpix.healpix_graph(4, mode="grid")
    elif name == "n8_nb20":
        A = healpix.healpix_graph(8, n_neighbors=20)
    elif name == "n8_cap":
        A = healpix.healpix_graph(8, indices=healpix.cap_indices(8))
    elif name == "asym":
        A = ref.asymmetric_graph()
    else:
        raise KeyError(name)
    rows, cols = ref.edges(A)
    nbr, nbrT = gnn_transformers.neighbour_tables(A)
    same = nbr is nbrT
    nbr = nbr.cuda()
    return A, rows, cols, nbr, (nbr if same else nbrT.cuda())


@functools.lru_cache(maxsize=None)
def inputs(M, d, seed=0, scale=1.0):
    rng = np.random.default_rng(seed)
    q, k, v, g = (rng.standard_normal((N, M, d)).astype(np.float32) for _ in range(4))
    return q * np.float32(scale), k * np.float32(scale), v, g


def run_forward(q, k, v, nbr, heads):
    out, lse = _native.nbr_attention(torch.as_tensor(q).cuda(), torch.as_tensor(k).cuda(), torch.as_tensor(v).cuda(), nbr, heads)
    torch.cuda.synchronize()
    return out.cpu().numpy(), lse.cpu().numpy()


def test_graph_shapes_are_the_ones_the_cases_name():
    lens = lambda name: (graph(name)[3] >= 0).sum(1).cpu().numpy()
    assert (lens("n4_knn").min(), lens("n4_knn").max()) == (8, 9)
    assert (lens("n4_grid").min(), lens("n4_grid").max()) == (7, 8)
    assert lens("n8_nb20").min() == 20 and lens("n8_nb20").max() == 22
    assert graph("n8_cap")[3].shape[0] == 260 and lens("n8_cap").min() == 8 and lens("n8_cap").max() == 11
    la = lens("asym")
    assert graph("asym")[3].shape[0] == 101 and la[5] == 0 and la[9] == 1 and la[17] == 40 and graph("asym")[3] is not graph("asym")[4]


@pytest.mark.parametrize("heads,depth", SHAPES)
@pytest.mark.parametrize("name", ["n4_knn", "n4_grid", "n8_nb20", "n8_cap"])
def test_forward_parity(name, heads, depth):
    _, rows, cols, nbr, _ = graph(name)
    q, k, v, _ = inputs(nbr.shape[0], heads * depth)
    want, s = ref.attention_np(q, k, v, rows, cols, heads)
    out, lse = run_forward(q, k, v, nbr, heads)
    # the log-sum-exp the backward reads, against the edge list's
    den = np.zeros((N, nbr.shape[0], heads))
    np.add.at(den, (slice(None), rows), np.exp(s))
    e_out, e_lse = rel_err(out, want), rel_err(lse, np.log(den))
    print(f"{name} heads {heads} depth {depth}: out {e_out:.2e} lse {e_lse:.2e}")
    assert e_out <= 1e-5 and e_lse <= 1e-5


@pytest.mark.parametrize("heads,depth", list(OTHER_DEPTHS))
@pytest.mark.parametrize("name", ["n4_knn", "n8_nb20", "n8_cap", "asym"])
def test_forward_parity_at_every_depth_and_lane_layout(name, heads, depth):
    """Depths 8 and 32 (head_sum over 2 and 8 lanes), depth 4 with several heads (no shuffle at all), rows of 2, 5, 6, 16 and 64
    lanes; ``asym`` adds the empty row, the one-neighbour row and the 40-wide row to each."""
    lpr, rpw = heads * depth // 4, 64 // (heads * depth // 4)
    assert (lpr, rpw) == OTHER_DEPTHS[(heads, depth)]
    _, rows, cols, nbr, _ = graph(name)
    M = nbr.shape[0]
    q, k, v, _ = inputs(M, heads * depth)
    want, s = ref.attention_np(q, k, v, rows, cols, heads)
    out, lse = run_forward(q, k, v, nbr, heads)
    den = np.zeros((N, M, heads))
    np.add.at(den, (slice(None), rows), np.exp(s))
    want_lse = np.log(np.where(den > 0, den, 1.0))  # (a row without neighbours: 0, as the kernel's header says)
    e_out, e_lse = rel_err(out, want), rel_err(lse, want_lse)
    print(f"{name} heads {heads} depth {depth} lpr {lpr} rpw {rpw}: out {e_out:.2e} lse {e_lse:.2e}")
    assert out.shape == (N, M, heads * depth) and lse.shape == (N, M, heads)
    assert e_out <= 1e-5 and e_lse <= 1e-5
    if name == "asym":
        assert (out[:, 5] == 0).all() and (lse[:, 5] == 0).all()  # the empty row, exactly


def test_strided_views_are_bitwise_the_contiguous_result():
    _, _, _, nbr, _ = graph("n4_knn")
    M, heads, depth = nbr.shape[0], 4, 16
    d = heads * depth
    buf = torch.as_tensor(np.random.default_rng(1).standard_normal((N, M, 3 * d)).astype(np.float32)).cuda()
    q, k, v = buf[..., :d], buf[..., d:2 * d], buf[..., 2 * d:]
    assert _native.rows_layout(k) == 3 * d and not k.is_contiguous()
    o_view, l_view = _native.nbr_attention(q, k, v, nbr, heads)
    o_copy, l_copy = _native.nbr_attention(q.contiguous(), k.contiguous(), v.contiguous(), nbr, heads)
    assert torch.equal(o_view, o_copy) and torch.equal(l_view, l_copy)
    # and through the differentiable op: views in, gradients equal to those of the copies
    g = torch.as_tensor(inputs(M, d)[3]).cuda()
    grads = []
    for make in (lambda t: t, lambda t: t.contiguous()):
        leaf = buf.clone().requires_grad_(True)
        out = gnn_transformers.scaled_dot_product_sparse_attention(make(leaf[..., :d]), make(leaf[..., d:2 * d]),
                                                                   make(leaf[..., 2 * d:]), nbr, nbr, heads)
        out.backward(g)
        grads.append(leaf.grad)
    assert torch.equal(grads[0], grads[1])


def test_large_logits_do_not_overflow():
    _, rows, cols, nbr, _ = graph("n4_knn")
    heads, depth = 2, 16
    q, k, v, _ = inputs(nbr.shape[0], heads * depth, seed=7, scale=6.0)
    want, s = ref.attention_np(q, k, v, rows, cols, heads)
    assert s.max() > 100 and np.isfinite(want).all()  # exp of the raw logit overflows in fp32 (above 88), not in float64
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(s.astype(np.float32))).any()
    out, lse = run_forward(q, k, v, nbr, heads)
    err = rel_err(out, want)
    print(f"logits in [{s.min():.0f}, {s.max():.0f}]: out {err:.2e}")
    assert np.isfinite(out).all() and np.isfinite(lse).all() and err <= 1e-4


@pytest.mark.parametrize("heads,depth", [(4, 16), (2, 64)])
def test_asymmetric_graph_forward(heads, depth):
    _, rows, cols, nbr, _ = graph("asym")
    q, k, v, _ = inputs(nbr.shape[0], heads * depth)
    want, _ = ref.attention_np(q, k, v, rows, cols, heads)
    out, lse = run_forward(q, k, v, nbr, heads)
    assert (out[:, 5] == 0).all() and (lse[:, 5] == 0).all()  # the empty row, exactly
    err = rel_err(out, want)
    print(f"asymmetric heads {heads} depth {depth}: out {err:.2e}")
    assert err <= 1e-5
    assert rel_err(out[:, 9], v[:, cols[rows == 9][0]]) <= 1e-6  # one neighbour: its v


@pytest.mark.parametrize("heads,depth", [(4, 16), (2, 64)])
@pytest.mark.parametrize("name", ["n4_knn", "n8_nb20", "asym"])
def test_backward_parity_and_reproducibility(name, heads, depth):
    _, rows, cols, nbr, nbrT = graph(name)
    q, k, v, g = inputs(nbr.shape[0], heads * depth)
    want = ref.attention_grads64(q, k, v, rows, cols, heads, g)
    runs = []
    for _ in range(2):
        t = [torch.as_tensor(a).cuda().requires_grad_(True) for a in (q, k, v)]
        out = gnn_transformers.scaled_dot_product_sparse_attention(t[0], t[1], t[2], nbr, nbrT, heads)
        out.backward(torch.as_tensor(g).cuda())
        torch.cuda.synchronize()
        runs.append([out.detach()] + [a.grad for a in t])
    errs = [rel_err(a.cpu().numpy(), b) for a, b in zip(runs[0], want)]
    print(f"{name} heads {heads} depth {depth}: out {errs[0]:.2e} dq {errs[1]:.2e} dk {errs[2]:.2e} dv {errs[3]:.2e}")
    assert errs[0] <= 1e-5 and max(errs[1:]) <= 2e-5
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)  # no atomics: bit for bit


@pytest.mark.parametrize("heads,depth", BACKWARD_OTHER_DEPTHS)
@pytest.mark.parametrize("name", ["n4_knn", "asym"])
def test_backward_parity_and_reproducibility_at_every_depth(name, heads, depth):
    """The backward at the depths 4, 8 and 32: same reference, same tolerances, same bit-for-bit repeat as the test above.
    On ``asym`` the second pass walks a table (nbrT) that is not the first pass's."""
    _, rows, cols, nbr, nbrT = graph(name)
    q, k, v, g = inputs(nbr.shape[0], heads * depth)
    want = ref.attention_grads64(q, k, v, rows, cols, heads, g)
    runs = []
    for _ in range(2):
        t = [torch.as_tensor(a).cuda().requires_grad_(True) for a in (q, k, v)]
        out = gnn_transformers.scaled_dot_product_sparse_attention(t[0], t[1], t[2], nbr, nbrT, heads)
        out.backward(torch.as_tensor(g).cuda())
        torch.cuda.synchronize()
        runs.append([out.detach()] + [a.grad for a in t])
    errs = [rel_err(a.cpu().numpy(), b) for a, b in zip(runs[0], want)]
    print(f"{name} heads {heads} depth {depth}: out {errs[0]:.2e} dq {errs[1]:.2e} dk {errs[2]:.2e} dv {errs[3]:.2e}")
    assert errs[0] <= 1e-5 and max(errs[1:]) <= 2e-5
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)  # no atomics: bit for bit
    if name == "asym":
        assert nbrT is not nbr and (runs[0][1][:, 5] == 0).all()  # dq of the row without neighbours


def test_misaligned_views_are_refused_before_any_launch():
    """Storage offset of one float, and a row stride that is no multiple of four floats: the kernels read 16 bytes per lane, so
    the C ABI refuses both, in the forward and in the backward, and launches nothing (the pre-filled outputs keep their
    contents).  ``_native.nbr_attention`` passes the refusal on as a ValueError.  The differentiable op copies what a copy
    can mend (the stride: a copy is a fresh, aligned allocation) and gives the contiguous call's bits; an offset view is
    already contiguous, ``.contiguous()`` returns it unchanged, and the op raises the C ABI's error."""
    _, _, _, nbr, nbrT = graph("asym")
    M, heads, depth = nbr.shape[0], 2, 8
    d = heads * depth
    q, k, v, g = (torch.as_tensor(a).cuda() for a in inputs(M, d))
    out, lse = _native.nbr_attention(q, k, v, nbr, heads)
    off = [offset_view(a, 1) for a in (q, k, v)]
    pad = [padded_view(a, 2) for a in (q, k, v)]
    assert _native.rows_layout(pad[0]) == d + 2 and (d + 2) % 4 != 0
    with pytest.raises(ValueError, match="must be 16-byte aligned"):
        _native.nbr_attention(off[0], off[1], off[2], nbr, heads)
    with pytest.raises(ValueError, match="row stride 18 must be a multiple of 4 floats"):
        _native.nbr_attention(pad[0], pad[1], pad[2], nbr, heads)
    with pytest.raises(ValueError, match="must be 16-byte aligned"):
        _native.nbr_attention_backward(off[0], off[1], off[2], out, lse, g, nbr, nbrT, heads)
    with pytest.raises(ValueError, match="row stride 18 must be a multiple of 4 floats"):
        _native.nbr_attention_backward(pad[0], pad[1], pad[2], out, lse, g, nbr, nbrT, heads)

    # the C ABI itself, on outputs filled beforehand
    L, p, stream = _native.lib(), _native._ptr, _native._stream_ptr(q.device)
    o_fill, l_fill = torch.full_like(out, 7.0), torch.full_like(lse, 7.0)
    grads = [torch.full_like(out, 7.0) for _ in range(3)]
    delta = torch.full_like(lse, 7.0)
    W, WT = int(nbr.shape[1]), int(nbrT.shape[1])
    for views, ld, text in ((off, d, "16-byte aligned"), (pad, d + 2, "multiple of 4 floats")):
        rc = L.dsph_nbr_attention_forward(p(views[0]), p(views[1]), p(views[2]), ld, p(o_fill), p(l_fill), p(nbr), W, N, M, heads, depth,
                                          0, stream)
        assert rc == -1 and text in _native.last_error()
        rc = L.dsph_nbr_attention_backward(p(views[0]), p(views[1]), p(views[2]), ld, p(out), p(lse), p(g), p(nbr), W, p(nbrT), WT,
                                           p(delta), p(grads[0]), p(grads[1]), p(grads[2]), d, N, M, heads, depth, 0, stream)
        assert rc == -1 and text in _native.last_error()
    # misaligned gradients, everything else in order
    goff = [offset_view(a, 1) for a in grads]
    rc = L.dsph_nbr_attention_backward(p(q), p(k), p(v), d, p(out), p(lse), p(g), p(nbr), W, p(nbrT), WT, p(delta), p(goff[0]),
                                       p(goff[1]), p(goff[2]), d, N, M, heads, depth, 0, stream)
    assert rc == -1 and "16-byte aligned" in _native.last_error()
    torch.cuda.synchronize()
    for t in [o_fill, l_fill, delta] + grads + goff:
        assert bool((t == 7.0).all())  # nothing ran

    # the differentiable op
    with pytest.raises(ValueError, match="must be 16-byte aligned"):
        gnn_transformers.scaled_dot_product_sparse_attention(off[0], off[1], off[2], nbr, nbrT, heads)
    results = []
    for src in ((q, k, v), pad):
        t = [a.detach().requires_grad_(True) for a in src]
        o = gnn_transformers.scaled_dot_product_sparse_attention(t[0], t[1], t[2], nbr, nbrT, heads)
        o.backward(g)
        results.append([o.detach()] + [a.grad for a in t])
    assert torch.equal(results[0][0], out)
    for a, b in zip(results[0], results[1]):
        assert torch.equal(a, b)  # the copies: bit for bit the contiguous call


def test_bad_shapes_raise():
    _, _, _, nbr, _ = graph("n4_knn")
    M = nbr.shape[0]
    t = torch.zeros((N, M, 24), device="cuda")
    with pytest.raises(ValueError, match="4, 8, 16, 32, 64"):
        _native.nbr_attention(t, t, t, nbr, 2)  # depth 12
    t = torch.zeros((N, M, 320), device="cuda")
    with pytest.raises(ValueError, match="256"):
        _native.nbr_attention(t, t, t, nbr, 5)
    t = torch.zeros((N, M + 1, 16), device="cuda")
    with pytest.raises(ValueError, match="rows"):
        _native.nbr_attention(t, t, t, nbr, 1)
    with pytest.raises(ValueError):
        gnn_transformers.scaled_dot_product_sparse_attention(t.cpu(), t.cpu(), t.cpu(), nbr, nbr, 1)


def _randomise(layer, seed):
    """Every parameter away from its special initial value (zero biases, unit gains), seeded."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in layer.named_parameters():
            r = torch.randn(p.shape, generator=gen)
            if name.endswith("bias") or "pos_embedding" in name:
                p.copy_((0.3 * r).to(p.device))
            elif "layer_norm" in name:
                p.copy_((1.0 + 0.2 * r).to(p.device))
            else:
                p.copy_((r / np.sqrt(p.shape[1])).to(p.device))


@pytest.mark.parametrize("layer_norm,positional_encoding", [(True, True), (False, True), (True, False)])
def test_graph_transformer_end_to_end(layer_norm, positional_encoding):
    A, rows, cols, _, _ = graph("n4_knn")
    M, Fin, key_dim, heads, n_layers = A.shape[0], 5, 8, 2, 2
    layer = gnn_transformers.Graph_Transformer(A, key_dim, heads, positional_encoding=positional_encoding, n_layers=n_layers,
                                               layer_norm=layer_norm)
    rng = np.random.default_rng(11)
    x = rng.standard_normal((N, M, Fin)).astype(np.float32)
    g = rng.standard_normal((N, M, key_dim * heads)).astype(np.float32)
    xg = torch.as_tensor(x).cuda()
    with torch.no_grad():
        layer(xg)  # builds the lazily created parameters
    _randomise(layer, 5)
    names = [n for n, _ in layer.named_parameters()]
    assert "embed.weight" in names and ("pos_encoder.pos_embedding" in names) == positional_encoding
    assert ("mha_layers.1.layer_norm2.weight" in names) == layer_norm and "mha_layers.1.wqkv.weight" in names
    out = layer(xg)
    assert tuple(out.shape) == (N, M, key_dim * heads)
    out.backward(torch.as_tensor(g).cuda())
    torch.cuda.synchronize()
    params = {n: p.detach().cpu().numpy() for n, p in layer.named_parameters()}
    kw = dict(rows=rows, cols=cols, num_heads=heads, n_layers=n_layers, positional_encoding=positional_encoding,
              layer_norm=layer_norm)
    out64, g64 = ref.graph_transformer_grads(x, params, g, torch.float64, **kw)
    out32, g32 = ref.graph_transformer_grads(x, params, g, torch.float32, **kw)
    got = {n: p.grad.cpu().numpy() for n, p in layer.named_parameters()}
    e_cpu, e_gpu = rel_err(out32, out64), rel_err(out.detach().cpu().numpy(), out64)
    print(f"norm {layer_norm} pos {positional_encoding}: output cpu-fp32 {e_cpu:.2e} gpu {e_gpu:.2e}")
    failed = [] if e_gpu <= 10 * e_cpu else [("output", e_gpu, e_cpu)]
    for n in names:
        e_cpu, e_gpu = rel_err(g32[n], g64[n]), rel_err(got[n], g64[n])
        print(f"  d {n}: cpu-fp32 {e_cpu:.2e} gpu {e_gpu:.2e}")
        if not e_gpu <= 10 * e_cpu:
            failed.append((n, e_gpu, e_cpu))
    assert not failed, f"more than ten times the CPU fp32 error: {failed}"


def test_healpy_gcnn_composition():
    model = deepsphere.HealpyGCNN(8, np.arange(768), [Healpy_Transformer(8, 2), HealpyPool(1), HealpyChebyshev(K=3, Fout=8)])
    x = torch.as_tensor(np.random.default_rng(2).standard_normal((N, 768, 3)).astype(np.float32)).cuda()
    with torch.no_grad():
        y = model(x)
        z = x
        for layer in model:
            z = layer(z)
    assert tuple(y.shape) == (N, 192, 8) and torch.isfinite(y).all()
    assert isinstance(model[0], gnn_transformers.Graph_Transformer) and model[0].nbr.is_cuda
    assert torch.equal(y, z)
    # and it trains: gradients reach the transformer's parameters through the pooling and the convolution
    model(x, training=True).square().sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model[0].parameters())
    assert float(model[0].mha_layers[0].wqkv.weight.grad.abs().max()) > 0
