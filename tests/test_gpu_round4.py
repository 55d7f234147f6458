"""Round-4 GPU tests (all through the C ABI): the parity gaps VERDICT r3 listed -- BASELINE configs[1] as bench.py times it,
the sharded form of configs[3] at its full size, the residual block against its oracle restatement on a k-NN graph --
the per-plan options that replaced the environment switches, the two-part launch finishing only its own rows, and
K > 5 through the product identity (passes of K <= 5 on the fast kernels)."""

import ctypes

import numpy as np
import pytest
import torch
from scipy import sparse

from deepsphere import _native, gnn_layers, healpix, utils
from helpers import rel_err
from oracle import cheb_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-5  # max|y - y_ref| <= 1e-5 max|y_ref| against the float64 oracle, whatever the arithmetic


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).cuda()


def _grid_ell(nside):
    import bench

    cols, vals, _ = bench.build_laplacian(nside, torch.device("cuda", 0))
    return cols, vals


def _csr(cols, vals):
    M, W = cols.shape
    return sparse.csr_matrix((vals.reshape(-1).astype(np.float64), cols.reshape(-1), np.arange(0, W * M + 1, W)), shape=(M, M))


# ---------------------------------------------------------------------------------------------------------------------
# BASELINE configs[1] exactly as `bench.py --config c2` times it
# ---------------------------------------------------------------------------------------------------------------------


def test_config2_as_benchmarked():
    """nside 256, K 5, 16 -> 32, batch 8, the layer default for 16 input channels (three-term split), fused kernels, bias + ReLU:
    the WHOLE map of every batch element against the float64 oracle (one map at a time: the op is batch independent)."""
    nside, N, Fin, Fout, K = 256, 8, 16, 32, 5
    assert gnn_layers.resolve_precision(gnn_layers.DEFAULT_PRECISION, Fin) == "bf16x3"
    cols, vals = _grid_ell(nside)
    M = cols.shape[0]
    plan = _native.LaplacianPlan(cols, vals, device=0)
    plan.prepare(K, Fin)
    n_struct, n_bfs = plan.tile_counts(K)
    assert n_struct == 3048 and n_bfs == 24, "every tile but the 24 at the sphere's 7-neighbour vertices is structured"
    gen = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn((N, M, Fin), device="cuda", generator=gen)
    rng = np.random.default_rng(13)
    W = (rng.standard_normal((Fin * K, Fout)) * orc.default_kernel_stddev(Fin, K)).astype(np.float32)
    b = rng.standard_normal(Fout).astype(np.float32)
    y, _ = _native.cheb_forward(plan, x, _dev(W), _dev(b), K, act=_native.ACT_RELU, precision=_native.PREC_BF16X3,
                                algo=_native.ALGO_FUSED)
    Lt = _csr(cols, vals)
    worst = 0.0
    for n in range(N):
        ref = orc.chebyshev_forward(Lt, x[n : n + 1].cpu().numpy(), W, K, bias=b, activation="relu")
        worst = max(worst, rel_err(y[n : n + 1].cpu().numpy(), ref))
    print(f"config 2 as benchmarked: {n_struct} + {n_bfs} tiles, worst map error {worst:.2e}")
    assert worst < TOL


# ---------------------------------------------------------------------------------------------------------------------
# the sharded form of BASELINE configs[3] at its full size, every rank's plan on the one GPU
# ---------------------------------------------------------------------------------------------------------------------


def test_config4_shards_at_full_size():
    """nside 2048, K 8, 32 -> 32, batch 1, split over 4 ranks (3 base pixels each, 7-ring halo): every rank's local plan run
    on this GPU with its halo rows taken from the global map must reproduce the unsharded rows BIT FOR BIT (DSPH_OPT_SPLIT =
    never on the unsharded plan, a plan with levels never splits).  Round 6: both sides run the K = 8 quad strips on the tiles
    whose 7-ring region stays inside a base pixel -- a rank owns whole base pixels, so its rectangles are the unsharded plan's
    and every output is summed in the same order -- and the breadth-first tile kernel on the base pixels' border tiles."""
    from deepsphere import sharding

    nside, N, Fin, Fout, K, world = 2048, 1, 32, 32, 8, 4
    cols, vals = _grid_ell(nside)
    M = cols.shape[0]
    gen = torch.Generator(device="cuda").manual_seed(4)
    x = torch.randn((N, M, Fin), device="cuda", generator=gen)
    rng = np.random.default_rng(44)
    W = _dev((rng.standard_normal((Fin * K, Fout)) * orc.default_kernel_stddev(Fin, K)).astype(np.float32))
    plan = _native.LaplacianPlan(cols, vals, device=0, options={_native.OPT_SPLIT: _native.SPLIT_NEVER})
    full, _ = _native.cheb_forward(plan, x, W, None, K, precision=_native.PREC_BF16X3, algo=_native.ALGO_FUSED)
    assert plan.strip_tiles(Fin, Fout, K, _native.PREC_BF16X3, N=N) >= 12 * (nside // 16 - 2) ** 2
    plan.close()
    for r in range(world):
        lay = sharding.ShardLayout(cols, vals, K, r, world)
        a, e = lay.own
        assert e - a == 3 * nside * nside and lay.n_cols > lay.n_own
        lp = _native.LaplacianPlan(lay.local_cols, lay.local_vals, n_cols=lay.n_cols, device=0, levels=lay.levels)
        assert lp.strip_tiles(Fin, Fout, K, _native.PREC_BF16X3, N=N) >= 3 * (nside // 16 - 2) ** 2, "the rank's base pixels' interiors on the strips"
        xl = x[:, torch.as_tensor(lay.local_ids).cuda()].contiguous()
        y, _ = _native.cheb_forward(lp, xl, W, None, K, precision=_native.PREC_BF16X3, algo=_native.ALGO_FUSED)
        same = bool(torch.equal(y, full[:, a:e]))
        print(f"rank {r}: rows [{a}, {e}), {lay.n_cols - lay.n_own} halo rows, equal {same}")
        assert same, f"rank {r}: a shard must reproduce the unsharded rows bit for bit"
        lp.close()
        del y, xl


# ---------------------------------------------------------------------------------------------------------------------
# VERDICT r3 item 2e / SURVEY 8 f2: the residual block against oracle.residual_forward on a graph that is not the identity
# ---------------------------------------------------------------------------------------------------------------------


def _set_norm(mod, rng, F):
    with torch.no_grad():
        p = {"gamma": rng.standard_normal(F) * 0.5 + 1.0, "beta": rng.standard_normal(F) * 0.3}
        mod.weight.copy_(torch.from_numpy(p["gamma"]).float())
        mod.bias.copy_(torch.from_numpy(p["beta"]).float())
        if isinstance(mod, torch.nn.BatchNorm1d):
            p["moving_mean"], p["moving_var"] = rng.standard_normal(F) * 0.2, rng.random(F) + 0.5
            mod.running_mean.copy_(torch.from_numpy(p["moving_mean"]).float())
            mod.running_var.copy_(torch.from_numpy(p["moving_var"]).float())
    return p


@pytest.mark.parametrize("layer_type,activation,act_before,alpha,norm", [
    ("CHEBY", "relu", False, 0.5, None),
    ("CHEBY", "elu", True, 0.25, None),
    ("CHEBY", None, False, 7.0, None),            # alpha ignored without an activation (gnn_layers.py:407-408)
    ("MONO", "tanh", False, 1.0, None),
    ("CHEBY", "relu", False, 1.0, "batch_norm"),  # Keras defaults: epsilon 1e-3, affine, moving statistics in inference
    ("CHEBY", "relu", True, 0.5, "layer_norm"),
])
def test_residual_block_against_the_oracle_on_a_knn_graph(layer_type, activation, act_before, alpha, norm):
    """GCNN_ResidualLayer (reference gnn_layers.py:312-413) on the reference's kind of graph -- symmetrised 8-nearest-neighbour
    HEALPix Laplacian, nside 16 -- with the sub-layers' own bias and activation: values against the float64 restatement
    (oracle.residual_forward), inference mode, skip connection through the one-pass HIP epilogue."""
    nside, N, F, K = 16, 3, 8, 4
    L = healpix.healpix_laplacian(nside, n_neighbors=8, mode="knn")
    M = L.shape[0]
    rng = np.random.default_rng(sum(map(ord, repr((layer_type, activation, act_before, norm)))))
    kw = {"L": L, "K": K, "use_bias": True, "activation": "relu", "device": "cuda:0", "precision": "bf16x6"}
    block = gnn_layers.GCNN_ResidualLayer(layer_type, kw, activation=activation, act_before=act_before, alpha=alpha,
                                          use_bn=norm is not None, norm_type=norm or "batch_norm")
    x = rng.standard_normal((N, M, F)).astype(np.float32)
    block.eval()
    with torch.no_grad():
        block(_dev(x))  # builds the sub-layers and the norm modules
        k1 = (rng.standard_normal((F * K, F)) * 0.3).astype(np.float32)
        k2 = (rng.standard_normal((F * K, F)) * 0.3).astype(np.float32)
        b1, b2 = rng.standard_normal(F).astype(np.float32) * 0.1, rng.standard_normal(F).astype(np.float32) * 0.1
        block.layer1.kernel.copy_(torch.from_numpy(k1))
        block.layer2.kernel.copy_(torch.from_numpy(k2))
        block.layer1.bias.copy_(torch.from_numpy(b1).reshape(1, 1, F))
        block.layer2.bias.copy_(torch.from_numpy(b2).reshape(1, 1, F))
        bn_params = (None, None)
        if norm is not None:
            bn_params = (_set_norm(block.bn1, rng, F), _set_norm(block.bn2, rng, F))
        y = block(_dev(x)).cpu().numpy()
    Lt, _ = orc.prepare_L(L, scale=0.75 if layer_type == "CHEBY" else 1.0)
    ref = orc.residual_forward(Lt, x, (k1, k2), K, layer_type=layer_type, layer_biases=(b1, b2), layer_activation="relu",
                               activation=activation, act_before=act_before, use_bn=norm is not None,
                               norm_type=norm or "batch_norm", bn_params=bn_params, training=False, alpha=alpha)
    err = rel_err(y, ref)
    print(f"residual {layer_type} act={activation} before={act_before} norm={norm}: err {err:.2e}")
    assert err < TOL


# ---------------------------------------------------------------------------------------------------------------------
# VERDICT r3 item 8 / ADVICE r3: plan options instead of environment switches; parts finish only their own rows
# ---------------------------------------------------------------------------------------------------------------------


def test_plan_options_replace_the_environment_switches():
    """dsph_plan_set_option: strips always / never fix the kernel choice independently of the batch; the structured and
    table switches move tiles between the kernels; bad values are DSPH_E_BADARG; every combination computes the same map
    to rounding."""
    nside, K, Fin, Fout = 128, 5, 64, 64
    cols, vals = _grid_ell(nside)
    M = cols.shape[0]
    rng = np.random.default_rng(9)
    x = _dev(rng.standard_normal((1, M, Fin)).astype(np.float32))
    W = _dev((rng.standard_normal((Fin * K, Fout)) * orc.default_kernel_stddev(Fin, K)).astype(np.float32))
    kw = dict(precision=_native.PREC_BF16X3, algo=_native.ALGO_FUSED)
    plan = _native.LaplacianPlan(cols, vals, device=0)
    assert plan.strip_tiles(Fin, Fout, K, N=1) == 0 and plan.strip_tiles(Fin, Fout, K, N=64) > 0  # the cost rule sees the batch
    y_auto, _ = _native.cheb_forward(plan, x, W, None, K, **kw)
    plan.set_option(_native.OPT_STRIPS, _native.STRIPS_ALWAYS)
    n_always = plan.strip_tiles(Fin, Fout, K, N=1)
    assert n_always > 0 and plan.strip_tiles(Fin, Fout, K, N=64) == n_always
    assert plan.strip_tiles(Fin, 96, K, N=1) == n_always and plan.strip_tiles(Fin, 32, K, N=1) == 0  # first 64-column block
    y_strips, _ = _native.cheb_forward(plan, x, W, None, K, **kw)
    plan.set_option(_native.OPT_STRIPS, _native.STRIPS_NEVER)
    assert plan.strip_tiles(Fin, Fout, K, N=64) == 0
    y_never, _ = _native.cheb_forward(plan, x, W, None, K, **kw)
    assert torch.equal(y_never, y_auto)  # one map at nside 128: the rule had left the strips out
    s = float(y_auto.abs().max())
    assert 0 < float((y_strips - y_auto).abs().max()) / s < 2 * TOL
    ns0, nb0 = plan.tile_counts(K)
    plan.set_option(_native.OPT_TABLES, 0)
    ns1, nb1 = plan.tile_counts(K)
    assert ns1 < ns0 and ns1 + nb1 == ns0 + nb0
    plan.set_option(_native.OPT_STRUCT, 0)
    assert plan.tile_counts(K) == (0, ns0 + nb0)
    y_bfs, _ = _native.cheb_forward(plan, x, W, None, K, **kw)
    assert float((y_bfs - y_auto).abs().max()) / s < 2 * TOL
    for opt, bad in ((_native.OPT_STRIPS, 3), (_native.OPT_STRIP_MINROWS, 1), (99, 0), (_native.OPT_SPLIT, -1),
                     (5, 0), (7, 1)):  # (5, 7: the retired STRIP_SEG / STRIP_GENERIC, unknown like 99)
        with pytest.raises(ValueError):
            plan.set_option(opt, bad)
    plan.set_option(_native.OPT_STRUCT, 1)
    plan.prepare(K, Fin, release_host=True)
    with pytest.raises(RuntimeError):
        plan.set_option(_native.OPT_TABLES, 1)  # the tables cannot be rebuilt any more
    plan.set_option(_native.OPT_FORK, 0)  # does not touch the tables: still allowed


@pytest.mark.parametrize("act", [_native.ACT_ELU, _native.ACT_TANH])
def test_parts_finish_only_their_own_rows(act):
    """with a deferred activation the BOUNDARY call used to run the elementwise pass over ALL output rows, so a
    repeated or lone BOUNDARY call re-applied it to interior rows.  Each part now finalises exactly its tiles: either order,
    repeated, or alone."""
    from deepsphere import sharding

    nside, K, Fin, Fout, N = 64, 5, 16, 32, 2
    cols, vals = _grid_ell(nside)
    lay = sharding.ShardLayout(cols, vals, K, 0, 2)
    plan = _native.LaplacianPlan(lay.local_cols, lay.local_vals, n_cols=lay.n_cols, device=0, levels=lay.levels)
    rng = np.random.default_rng(31)
    x = _dev(rng.standard_normal((N, lay.n_cols, Fin)).astype(np.float32))
    W = _dev((rng.standard_normal((Fin * K, Fout)) * orc.default_kernel_stddev(Fin, K)).astype(np.float32))
    b = _dev(rng.standard_normal(Fout).astype(np.float32))
    kw = dict(act=act, precision=_native.PREC_BF16X3, algo=_native.ALGO_FUSED)
    whole, ws = _native.cheb_forward(plan, x, W, b, K, **kw)
    out = torch.full_like(whole, float("nan"))
    for part in (_native.PART_BOUNDARY, _native.PART_BOUNDARY, _native.PART_INTERIOR, _native.PART_INTERIOR):
        _native.cheb_forward(plan, x, W, b, K, part=part, out=out, workspace=ws, **kw)
    assert torch.equal(out, whole)
    lone = torch.full_like(whole, float("nan"))
    _native.cheb_forward(plan, x, W, b, K, part=_native.PART_BOUNDARY, out=lone, workspace=ws, **kw)
    wrote = ~torch.isnan(lone)
    assert bool(wrote.any()) and not bool(wrote.all())
    assert torch.equal(lone[wrote], whole[wrote])  # the rows it wrote are final, the others untouched


def test_backward_precision_is_resolved_per_contraction():
    """"auto" used the layer's forward Fin for the input gradient too.  A 64 -> 4 layer runs its forward in the
    three-term split and its dx (a contraction over 4 * K inputs) in the six-term split; gradients against the float64
    oracle at the default, 1e-5 for dx, 2e-5 for dkernel."""
    assert gnn_layers.resolve_precision("auto", 64) == "bf16x3" and gnn_layers.resolve_precision("auto", 4) == "bf16x6"
    assert gnn_layers.resolve_wgrad_precision("auto", 49152) == "bf16x3" and gnn_layers.resolve_wgrad_precision("auto", 768) == "fp32"
    assert gnn_layers.resolve_wgrad_precision("bf16x6", 10 ** 6) == "fp32"
    nside, N, Fin, Fout, K = 32, 2, 64, 4, 5
    L = healpix.healpix_laplacian(nside, mode="grid")
    Lt, _ = orc.prepare_L(L)
    cols, vals = utils.csr_to_ell(Lt)
    rng = np.random.default_rng(77)
    W = (rng.standard_normal((Fin * K, Fout)) * orc.default_kernel_stddev(Fin, K)).astype(np.float32)
    layer = gnn_layers.Chebyshev.from_prepared_ell(cols, vals, K, Fout=Fout, device="cuda:0",
                                                   initializer=lambda t: t.copy_(torch.from_numpy(W)))
    x = rng.standard_normal((N, Lt.shape[0], Fin)).astype(np.float32)
    dy = rng.standard_normal((N, Lt.shape[0], Fout)).astype(np.float32)
    xt = _dev(x).requires_grad_(True)
    y = layer(xt)
    y.backward(_dev(dy))
    dx_ref, dW_ref = orc.chebyshev_backward(Lt, x, W, K, dy)
    e_dx, e_dw = rel_err(xt.grad.cpu().numpy(), dx_ref), rel_err(layer.kernel.grad.cpu().numpy(), dW_ref)
    print(f"64 -> 4 at the default: dx err {e_dx:.2e}, dkernel err {e_dw:.2e}")
    assert e_dx < TOL and e_dw < 2 * TOL


# ---------------------------------------------------------------------------------------------------------------------
# K > 5 through T_{4+j} = 2 T_4 T_j - T_{|4-j|}: passes of K <= 5 on the fast kernels
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("prec,tol", [("fp32", 2e-6), ("bf16x6", 2e-6), ("bf16x3", TOL)])
@pytest.mark.parametrize("nside,N,Fin,Fout,K,basis", [
    (64, 2, 32, 32, 8, "chebyshev"),    # BASELINE configs[3]'s channel counts and order: two passes (K 4, then K 5 on [x, u])
    (64, 1, 16, 32, 10, "chebyshev"),   # the reference tutorials' K = 10 (examples/quick_start.ipynb:118-127): three passes
    (64, 2, 8, 24, 6, "chebyshev"),     # K = 6: the inner pass is a single step
    (64, 1, 4, 12, 13, "chebyshev"),    # three passes of K = 5
    (128, 1, 32, 32, 8, "chebyshev"),   # several tiles per workgroup
    (64, 2, 16, 16, 9, "monomial"),     # the other basis: L^{4+j} = L^4 L^j
    (64, 1, 3, 5, 7, "chebyshev"),      # channel counts that get padded
    (64, 1, 16, 16, 17, "chebyshev"),   # K > 13: the terms of the inner levels are no longer plain slices of the kernel
])
def test_high_order_through_the_product_identity(nside, N, Fin, Fout, K, basis, prec, tol):
    """Whole maps against the float64 oracle with the split route forced (DSPH_OPT_SPLIT = always), bias + ReLU in the last
    pass; and against the breadth-first-table kernel's result for K <= 10."""
    cols, vals = _grid_ell(nside)
    M = cols.shape[0]
    rng = np.random.default_rng(nside + Fin + Fout + K)
    x = rng.standard_normal((N, M, Fin)).astype(np.float32)
    W = (rng.standard_normal((Fin * K, Fout)) * orc.default_kernel_stddev(Fin, K)).astype(np.float32)
    b = rng.standard_normal(Fout).astype(np.float32)
    fwd = orc.chebyshev_forward if basis == "chebyshev" else orc.monomial_forward
    ref = fwd(_csr(cols, vals), x, W, K, bias=b, activation="relu")
    P = {"fp32": _native.PREC_FP32, "bf16x3": _native.PREC_BF16X3, "bf16x6": _native.PREC_BF16X6}[prec]
    B = {"chebyshev": _native.BASIS_CHEBYSHEV, "monomial": _native.BASIS_MONOMIAL}[basis]
    plan = _native.LaplacianPlan(cols, vals, device=0, options={_native.OPT_SPLIT: _native.SPLIT_ALWAYS})
    y, ws = _native.cheb_forward(plan, _dev(x), _dev(W), _dev(b), K, act=_native.ACT_RELU, precision=P, basis=B)
    err = rel_err(y.cpu().numpy(), ref)
    y2, _ = _native.cheb_forward(plan, _dev(x), _dev(W), _dev(b), K, act=_native.ACT_RELU, precision=P, basis=B, workspace=ws)
    assert torch.equal(y, y2)
    msg = f"split nside={nside} {Fin}->{Fout} K={K} {basis} {prec}: err {err:.2e}"
    if K <= 10:  # (K = 10: the 9-ring regions of round 6, 1,156 rows in planes of 1,168)
        plain = _native.LaplacianPlan(cols, vals, device=0, options={_native.OPT_SPLIT: _native.SPLIT_NEVER})
        yb, _ = _native.cheb_forward(plain, _dev(x), _dev(W), _dev(b), K, act=_native.ACT_RELU, precision=P, basis=B)
        eb = rel_err(yb.cpu().numpy(), ref)
        msg += f" (breadth-first-table kernel: {eb:.2e})"
        assert eb < (2 * tol if (prec == "bf16x3" and Fin < 16) else tol)
    print(msg)
    # (the three-term split with fewer than 16 input channels has no 1e-5 guarantee -- a handful of products per output --
    # and no layer uses it there unless asked: held to 2e-5 like tools/fuzz_gpu.py does; with four passes,
    # K > 13, every pass re-rounds its input to bf16 hi + lo: 2e-5 there too)
    assert err < (2 * tol if (prec == "bf16x3" and (Fin < 16 or K > 13)) else tol)


def test_high_order_layer_like_the_tutorials():
    """HealpyChebyshev(K=10, ...) as in examples/quick_start.ipynb:118-127, through the layer API at its defaults, forward and
    gradients (the backward runs the same split on dy; the weight gradient its own kernels)."""
    nside, N, Fin, Fout, K = 32, 2, 16, 8, 10
    L = healpix.healpix_laplacian(nside, mode="grid")
    Lt, _ = orc.prepare_L(L)
    cols, vals = utils.csr_to_ell(Lt)
    rng = np.random.default_rng(10)
    W = (rng.standard_normal((Fin * K, Fout)) * orc.default_kernel_stddev(Fin, K)).astype(np.float32)
    layer = gnn_layers.Chebyshev.from_prepared_ell(cols, vals, K, Fout=Fout, device="cuda:0", activation="elu", use_bias=True,
                                                   initializer=lambda t: t.copy_(torch.from_numpy(W)))
    x = rng.standard_normal((N, Lt.shape[0], Fin)).astype(np.float32)
    with torch.no_grad():
        y = layer(_dev(x))
        bias = layer.bias.detach().cpu().numpy().reshape(-1)
    ref = orc.chebyshev_forward(Lt, x, W, K, bias=bias, activation="elu")
    assert rel_err(y.cpu().numpy(), ref) < TOL
    xt = _dev(x).requires_grad_(True)
    lin = gnn_layers.Chebyshev.from_prepared_ell(cols, vals, K, Fout=Fout, device="cuda:0",
                                                 initializer=lambda t: t.copy_(torch.from_numpy(W)))
    dy = rng.standard_normal((N, Lt.shape[0], Fout)).astype(np.float32)
    lin(xt).backward(_dev(dy))
    dx_ref, dW_ref = orc.chebyshev_backward(Lt, x, W, K, dy)
    assert rel_err(xt.grad.cpu().numpy(), dx_ref) < 2 * TOL
    assert rel_err(lin.kernel.grad.cpu().numpy(), dW_ref) < 2 * TOL


# ---------------------------------------------------------------------------------------------------------------------
# small-map latency -- weight images kept between forwards, the forward as one graph launch
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("Fin,Fout,K", [(1, 16, 5), (16, 96, 5), (16, 32, 10)])
def test_kept_weight_images_and_graph_replay(Fin, Fout, K):
    """DSPH_FWD_KEEP_WEIGHTS through the layer: the second and later inference forwards launch no weight-preparation kernel
    and give the same bits; an in-place update of the kernel (its version counter moves) re-packs; graph=True replays the
    same bits from one graph launch, follows weight updates and new inputs.  (1 -> 16: BASELINE configs[0]; 96 columns: two
    column blocks, each with its own image area; K = 10: the split route's per-pass areas.)"""
    nside, N = 64, 2
    cols, vals = _grid_ell(nside)
    M = cols.shape[0]
    rng = np.random.default_rng(Fin + Fout + K)
    W = (rng.standard_normal((Fin * K, Fout)) * orc.default_kernel_stddev(Fin, K)).astype(np.float32)
    mk = lambda **kw: gnn_layers.Chebyshev.from_prepared_ell(  # noqa: E731
        cols, vals, K, Fout=Fout, device="cuda:0", activation="relu", use_bias=True,
        initializer=lambda t: t.copy_(torch.from_numpy(W)), **kw)
    layer, glayer = mk(), mk(graph=True)
    x = _dev(rng.standard_normal((N, M, Fin)).astype(np.float32))
    Lt = _csr(cols, vals)
    with torch.no_grad():
        glayer(x)
        layer(x)  # (both built: the biases are random, make them the same)
        glayer.bias.copy_(layer.bias)
        y0 = layer(x).clone()
        assert layer._wkey is not None
        y1 = layer(x).clone()   # weight images kept
        y2 = layer(x).clone()
        assert torch.equal(y0, y1) and torch.equal(y0, y2)
        ref = orc.chebyshev_forward(Lt, x.cpu().numpy(), W, K, bias=layer.bias.cpu().numpy().reshape(-1), activation="relu")
        assert rel_err(y0.cpu().numpy(), ref) < 2 * TOL
        g0 = glayer(x).clone()
        g1 = glayer(x).clone()  # replay
        assert torch.equal(g0, y0) and torch.equal(g1, y0)
        # a weight update moves the version counter: both layers re-pack (the graph is re-captured)
        layer.kernel.mul_(0.5)
        glayer.kernel.mul_(0.5)
        y3 = layer(x).clone()
        ref3 = orc.chebyshev_forward(Lt, x.cpu().numpy(), 0.5 * W, K, bias=layer.bias.cpu().numpy().reshape(-1), activation="relu")
        assert rel_err(y3.cpu().numpy(), ref3) < 2 * TOL and not torch.equal(y3, y0)
        assert torch.equal(glayer(x), y3)
        # new contents in the same input buffer: the replay reads them; a new buffer: re-captured
        x.mul_(-1.0)
        y4 = layer(x).clone()
        assert torch.equal(glayer(x), y4)
        x2 = x.clone()
        assert torch.equal(glayer(x2), y4)


# ---------------------------------------------------------------------------------------------------------------------
# the callers either side of the convolution on the device -- pseudo-convolutions as GEMMs (the NEST pooling
# kernels: tests/test_gpu_pooling.py)
# ---------------------------------------------------------------------------------------------------------------------


def test_pseudo_convolutions_against_the_oracle():
    """HealpyPseudoConv / HealpyPseudoConv_Transpose (healpy_layers.py:88-216) as single GEMMs on the free reshaped views,
    against the oracle restatements with the weights mapped to the Keras layouts."""
    from deepsphere import healpy_layers

    rng = np.random.default_rng(12)
    N, M, Fin, Fout, p = 2, 768, 6, 10, 1
    x = rng.standard_normal((N, M, Fin)).astype(np.float32)
    pc = healpy_layers.HealpyPseudoConv(p, Fout).cuda()
    with torch.no_grad():
        y = pc(_dev(x))
        pc.filter.bias.normal_()
        y = pc(_dev(x))
        k = pc.filter.weight.permute(2, 1, 0).cpu().numpy()  # torch (Fout, Fin, 4^p) -> Keras (4^p, Fin, Fout)
        ref = orc.healpy_pseudo_conv(x.astype(np.float64), k.astype(np.float64), pc.filter.bias.cpu().numpy().astype(np.float64), p)
    assert rel_err(y.cpu().numpy(), ref) < 1e-5
    pt = healpy_layers.HealpyPseudoConv_Transpose(p, Fout).cuda()
    with torch.no_grad():
        z = pt(_dev(x))
        pt.filter.bias.normal_()
        z = pt(_dev(x))
        kt = pt.filter.weight.permute(2, 1, 0).cpu().numpy()  # torch (Fin, Fout, 4^p) -> (4^p, Fout, Fin)
        reft = orc.healpy_pseudo_conv_transpose(x.astype(np.float64), kt.astype(np.float64), pt.filter.bias.cpu().numpy().astype(np.float64), p)
    assert z.shape == (N, 4 * M, Fout) and rel_err(z.cpu().numpy(), reft) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# a fast kernel for the shapes a network starts with -- the input-side strip kernel (Fin <= 16)
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("prec", ["fp32", "bf16x3", "bf16x6"])
@pytest.mark.parametrize("nside,N,Fin,Fout,K,basis,act", [
    (128, 2, 16, 32, 5, "chebyshev", "relu"),   # BASELINE configs[1]'s channel counts
    (128, 3, 1, 16, 5, "chebyshev", None),      # configs[0]'s: one input channel (zero-padded to four), CH = 4
    (128, 1, 8, 64, 4, "chebyshev", "relu"),    # CH = 4 with both halves, two 32-column blocks, K = 4
    (128, 2, 12, 40, 3, "chebyshev", "elu"),    # three quads, a ragged second block, deferred activation, K = 3
    (128, 2, 4, 20, 2, "chebyshev", None),      # K = 2, a narrow block
    (128, 1, 16, 96, 5, "monomial", "relu"),    # the other basis, three column blocks over two 64-column launches
    (256, 2, 5, 24, 5, "chebyshev", "tanh"),    # padded channel count, larger map
    (128, 4, 4, 8, 5, "chebyshev", "relu"),     # the reference's own test network (4 -> 8 behind a pseudo-convolution): two maps per wave
    (128, 3, 3, 16, 4, "monomial", "elu"),      # pairs with a padded channel count, an odd batch, the other basis
    (128, 1, 4, 12, 5, "chebyshev", None),      # a single map in pair mode (its partner masked)
    (128, 3, 8, 8, 5, "chebyshev", "relu"),     # 8 -> 8: the class-T tiles beside the strips run two maps per item
    (128, 4, 7, 32, 4, "monomial", None),       # padded to eight channels, 32 columns
])
def test_input_side_strip_kernel_whole_map(nside, N, Fin, Fout, K, basis, act, prec):
    """Whole maps against the float64 oracle: the rectangles on cheb_istrip_kernel, the rest on the tile kernels; the kernel
    must really have been used, must be deterministic, and must equal the same plan with DSPH_OPT_STRIPS = never to rounding."""
    cols, vals = _grid_ell(nside)
    M = cols.shape[0]
    plan = _native.LaplacianPlan(cols, vals, device=0)
    n_strip = plan.strip_tiles(Fin, Fout, K, N=N)
    n_struct, n_bfs = plan.tile_counts(K)
    assert 0 < n_strip <= n_struct, "the rectangles of this map go to the input-side strip kernel"
    rng = np.random.default_rng(nside + Fin + Fout + K)
    x = rng.standard_normal((N, M, Fin)).astype(np.float32)
    W = (rng.standard_normal((Fin * K, Fout)) * orc.default_kernel_stddev(Fin, K)).astype(np.float32)
    b = rng.standard_normal(Fout).astype(np.float32)
    fwd = orc.chebyshev_forward if basis == "chebyshev" else orc.monomial_forward
    ref = fwd(_csr(cols, vals), x, W, K, bias=b, activation=act)
    P = {"fp32": _native.PREC_FP32, "bf16x3": _native.PREC_BF16X3, "bf16x6": _native.PREC_BF16X6}[prec]
    B = {"chebyshev": _native.BASIS_CHEBYSHEV, "monomial": _native.BASIS_MONOMIAL}[basis]
    A = {None: _native.ACT_NONE, "relu": _native.ACT_RELU, "elu": _native.ACT_ELU, "tanh": _native.ACT_TANH}[act]
    y, ws = _native.cheb_forward(plan, _dev(x), _dev(W), _dev(b), K, act=A, precision=P, algo=_native.ALGO_FUSED, basis=B)
    err = rel_err(y.cpu().numpy(), ref)
    tol = (2e-6 if prec != "bf16x3" else (TOL if Fin >= 16 else 2 * TOL)) * (5 if act == "tanh" else 1)
    print(f"istrip nside={nside} {Fin}->{Fout} K={K} {basis} {act} {prec}: {n_strip} strip tiles of {n_struct} + {n_bfs}, err {err:.2e}")
    assert err < tol
    y2, _ = _native.cheb_forward(plan, _dev(x), _dev(W), _dev(b), K, act=A, precision=P, algo=_native.ALGO_FUSED, basis=B, workspace=ws)
    assert torch.equal(y, y2)
    plain = _native.LaplacianPlan(cols, vals, device=0, options={_native.OPT_STRIPS: _native.STRIPS_NEVER})
    assert plain.strip_tiles(Fin, Fout, K, N=N) == 0
    y3, _ = _native.cheb_forward(plain, _dev(x), _dev(W), _dev(b), K, act=A, precision=P, algo=_native.ALGO_FUSED, basis=B)
    assert rel_err(y.cpu().numpy(), y3.cpu().numpy()) < 2 * tol


@pytest.mark.parametrize("prec", ["fp32", "bf16x3", "bf16x6"])
@pytest.mark.parametrize("nside,N,Fin,Fout,K,basis,act", [
    (128, 2, 1, 32, 5, "chebyshev", "relu"),    # a first layer: one channel, five levels in the inner index
    (128, 3, 2, 16, 5, "chebyshev", None),      # two channels: one per lane half
    (128, 1, 1, 64, 4, "chebyshev", "elu"),     # K = 4, two 32-column blocks, deferred activation
    (128, 2, 2, 40, 3, "monomial", "relu"),     # K = 3, the other basis, a ragged second block
    (128, 5, 1, 8, 2, "chebyshev", None),       # K = 2 (T_0 keeps three rows all the same), an odd batch: two maps per wave, one left over
    (128, 4, 1, 16, 5, "chebyshev", "relu"),    # 1 -> 16, the first layer of the networks: pairs of maps share a wave
    (128, 3, 1, 12, 4, "monomial", "elu"),      # pairs with a ragged width and the other basis
    (256, 2, 1, 96, 5, "monomial", "tanh"),     # larger map, three blocks over two 64-column launches
])
def test_level_packed_strip_kernel_for_one_and_two_channels(nside, N, Fin, Fout, K, basis, act, prec):
    """cheb_istrip1_kernel (layers with one or two input channels: the Chebyshev levels in the MFMA's inner index, one
    contraction per row) against the float64 oracle, deterministic, and equal to the tile kernels alone to rounding."""
    cols, vals = _grid_ell(nside)
    M = cols.shape[0]
    plan = _native.LaplacianPlan(cols, vals, device=0)
    assert plan.strip_tiles(Fin, Fout, K, N=N) > 0
    rng = np.random.default_rng(7 * nside + Fin + Fout + K)
    x = rng.standard_normal((N, M, Fin)).astype(np.float32)
    W = (rng.standard_normal((Fin * K, Fout)) * orc.default_kernel_stddev(Fin, K)).astype(np.float32)
    b = rng.standard_normal(Fout).astype(np.float32)
    fwd = orc.chebyshev_forward if basis == "chebyshev" else orc.monomial_forward
    ref = fwd(_csr(cols, vals), x, W, K, bias=b, activation=act)
    P = {"fp32": _native.PREC_FP32, "bf16x3": _native.PREC_BF16X3, "bf16x6": _native.PREC_BF16X6}[prec]
    B = {"chebyshev": _native.BASIS_CHEBYSHEV, "monomial": _native.BASIS_MONOMIAL}[basis]
    A = {None: _native.ACT_NONE, "relu": _native.ACT_RELU, "elu": _native.ACT_ELU, "tanh": _native.ACT_TANH}[act]
    y, ws = _native.cheb_forward(plan, _dev(x), _dev(W), _dev(b), K, act=A, precision=P, algo=_native.ALGO_FUSED, basis=B)
    err = rel_err(y.cpu().numpy(), ref)
    tol = (2e-6 if prec != "bf16x3" else 2 * TOL) * (5 if act == "tanh" else 1)
    print(f"istrip1 nside={nside} {Fin}->{Fout} K={K} {basis} {act} {prec}: err {err:.2e}")
    assert err < tol
    y2, _ = _native.cheb_forward(plan, _dev(x), _dev(W), _dev(b), K, act=A, precision=P, algo=_native.ALGO_FUSED, basis=B, workspace=ws)
    assert torch.equal(y, y2)
    plain = _native.LaplacianPlan(cols, vals, device=0, options={_native.OPT_STRIPS: _native.STRIPS_NEVER})
    y3, _ = _native.cheb_forward(plain, _dev(x), _dev(W), _dev(b), K, act=A, precision=P, algo=_native.ALGO_FUSED, basis=B)
    assert rel_err(y.cpu().numpy(), y3.cpu().numpy()) < 2 * tol
    # a map's result does not depend on the batch it came in (other row segments: same sums) -- bit for bit with
    # DSPH_OPT_PACK = 0; by default the tile kernels next to the strips pack four maps of so narrow a layer into one item when
    # the batch has more than one: equal to rounding
    y1, _ = _native.cheb_forward(plan, _dev(x[:1]), _dev(W), _dev(b), K, act=A, precision=P, algo=_native.ALGO_FUSED, basis=B)
    assert rel_err(y1.cpu().numpy(), y[:1].cpu().numpy()) < tol
    nopack = _native.LaplacianPlan(cols, vals, device=0, options={_native.OPT_PACK: 0})
    yn, _ = _native.cheb_forward(nopack, _dev(x), _dev(W), _dev(b), K, act=A, precision=P, algo=_native.ALGO_FUSED, basis=B)
    yn1, _ = _native.cheb_forward(nopack, _dev(x[:1]), _dev(W), _dev(b), K, act=A, precision=P, algo=_native.ALGO_FUSED, basis=B)
    assert torch.equal(yn1, yn[:1])
    assert rel_err(yn.cpu().numpy(), ref) < tol


def test_input_side_strip_kernel_partial_sky_and_batches():
    """A cap of the sphere at nside 256 (ragged rectangles), 16 -> 32, at batch sizes that change the row-segment count the
    kernel is launched with (1, 2, 5, 16 maps): every batch equals the oracle, and a map's result does not depend on the batch
    it came in (the segments only move where a strip's run-in rows lie: same sums, same bits)."""
    import bench

    nside, K, Fin, Fout = 256, 5, 16, 32
    cols, vals, _ = bench.build_laplacian_masked(nside, torch.device("cuda", 0))
    M = cols.shape[0]
    plan = _native.LaplacianPlan(cols, vals, device=0)
    assert plan.strip_tiles(Fin, Fout, K, N=1) > 0
    rng = np.random.default_rng(256)
    x = rng.standard_normal((16, M, Fin)).astype(np.float32)
    W = (rng.standard_normal((Fin * K, Fout)) * orc.default_kernel_stddev(Fin, K)).astype(np.float32)
    Lt = _csr(cols, vals)
    ref = orc.chebyshev_forward(Lt, x[:2], W, K)
    y16, _ = _native.cheb_forward(plan, _dev(x), _dev(W), None, K, precision=_native.PREC_BF16X3, algo=_native.ALGO_FUSED)
    assert rel_err(y16[:2].cpu().numpy(), ref) < TOL
    for N in (1, 2, 5):
        yN, _ = _native.cheb_forward(plan, _dev(x[:N]), _dev(W), None, K, precision=_native.PREC_BF16X3, algo=_native.ALGO_FUSED)
        assert torch.equal(yN, y16[:N]), f"batch {N}"


@pytest.mark.parametrize("Fin,Fout", [(16, 32), (1, 32), (1, 16), (4, 8)])
def test_input_side_strips_in_a_two_part_launch(Fin, Fout):
    """A rank's plan at nside 128 (two ranks): the interior part runs the strips, the boundary part the tile kernels; the two
    parts together equal the single launch bit for bit, with a deferred activation.  Fin = 1: a sharded first layer, the
    level-packed kernel; with at most 16 columns two maps per wave (an odd batch of three: one wave carries a single map)."""
    from deepsphere import sharding

    nside, K, N = 128, 5, 3
    cols, vals = _grid_ell(nside)
    lay = sharding.ShardLayout(cols, vals, K, 1, 2)
    plan = _native.LaplacianPlan(lay.local_cols, lay.local_vals, n_cols=lay.n_cols, device=0, levels=lay.levels)
    assert plan.strip_tiles(Fin, Fout, K, N=N) > 0
    rng = np.random.default_rng(41)
    x = _dev(rng.standard_normal((N, lay.n_cols, Fin)).astype(np.float32))
    W = _dev((rng.standard_normal((Fin * K, Fout)) * orc.default_kernel_stddev(Fin, K)).astype(np.float32))
    b = _dev(rng.standard_normal(Fout).astype(np.float32))
    kw = dict(act=_native.ACT_ELU, precision=_native.PREC_BF16X3 if Fin >= 16 else _native.PREC_BF16X6, algo=_native.ALGO_FUSED)
    whole, ws = _native.cheb_forward(plan, x, W, b, K, **kw)
    out = torch.full_like(whole, float("nan"))
    _native.cheb_forward(plan, x, W, b, K, part=_native.PART_INTERIOR, out=out, workspace=ws, **kw)
    _native.cheb_forward(plan, x, W, b, K, part=_native.PART_BOUNDARY, out=out, workspace=ws, **kw)
    assert torch.equal(out, whole)
    # and against the oracle on the rank's own rows
    full_x = np.zeros((N, cols.shape[0], Fin), dtype=np.float32)
    full_x[:, lay.local_ids] = x.cpu().numpy()
    ref = orc.chebyshev_forward(_csr(cols, vals), full_x, W.cpu().numpy(), K, bias=b.cpu().numpy(), activation="elu")
    a, e = lay.own
    assert rel_err(whole.cpu().numpy(), ref[:, a:e]) < TOL


def test_fuzz_input_side_strips_and_pass_chains():
    """A short run of tools/fuzz_gpu.py in its round-4 mode (FUZZ_ISTRIPS=1: random shapes of the input-side strip kernel on
    nside-128 grids and caps, every third case K 6..13 through the chain of passes), all three arithmetics against the unfused
    kernels."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, FUZZ_ISTRIPS="1")
    res = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_gpu.py"), "12", "7"], capture_output=True, text=True,
                         timeout=900, env=env)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "ALL OK" in res.stdout


# ---------------------------------------------------------------------------------------------------------------------
# the reference's 20-neighbour graphs -- every recurrence step through LDS tiles (cheb_tstep.hip)
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("nside,k,N,F,K,basis", [
    (32, 20, 3, 16, 5, "chebyshev"),   # ELL width 23 -> the 24-wide instantiation; one 16-channel slice
    (32, 20, 2, 40, 4, "chebyshev"),   # three slices, the last one partial
    (16, 20, 2, 4, 3, "monomial"),     # one 4-channel chunk, the other basis, 12 tiles
    (32, 20, 2, 5, 6, "chebyshev"),    # five channels (the quick-start model's width): scalar loads and stores; K = 6
    (16, 20, 3, 1, 10, "chebyshev"),   # one channel, the tutorials' K = 10
    (32, 8, 2, 8, 5, "chebyshev"),     # width 11: the fused kernels' territory -- the tiled step is not used, same answer
])
def test_tiled_step_on_wide_graphs(nside, k, N, F, K, basis):
    """A symmetrised k-nearest-neighbour graph as the reference's models build it: single steps through dsph_cheb_step with the
    tiled kernel and with the gather kernel (DSPH_OPT_TSTEP = 0) agree to rounding (the tiled kernel deals a row's slots by
    bank residue: the same terms in another order) and repeat bit for bit, the whole forward agrees with the float64 oracle, and
    so does the weight gradient (its planes come from the same steps)."""
    L = healpix.healpix_laplacian(nside, n_neighbors=k, mode="knn")
    Lt, _ = orc.prepare_L(L, scale=0.75 if basis == "chebyshev" else 1.0)
    cols, vals = utils.csr_to_ell(Lt)
    M, W_ell = cols.shape
    assert (W_ell > 12) == (k == 20)
    rng = np.random.default_rng(nside + k + F)
    x = rng.standard_normal((N, M, F)).astype(np.float32)
    plan = _native.LaplacianPlan(cols, vals, device=0)
    plain = _native.LaplacianPlan(cols, vals, device=0, options={_native.OPT_TSTEP: 0})
    xd, pd = _dev(x), _dev(rng.standard_normal((N, M, F)).astype(np.float32))
    a = _native.cheb_step(plan, xd, None, 1.0, 0.0)
    b = _native.cheb_step(plain, xd, None, 1.0, 0.0)
    assert rel_err(a.cpu().numpy(), b.cpu().numpy()) < 1e-6 and torch.equal(a, _native.cheb_step(plan, xd, None, 1.0, 0.0))
    if W_ell <= 12:
        assert torch.equal(a, b)  # (not a wide graph: both plans run the gather kernel)
    a2 = _native.cheb_step(plan, a, pd, 2.0, 1.0)
    b2 = _native.cheb_step(plain, a, pd, 2.0, 1.0)
    assert rel_err(a2.cpu().numpy(), b2.cpu().numpy()) < 1e-6
    ref1 = (Lt.astype(np.float64) @ x.transpose(1, 0, 2).reshape(M, -1)).reshape(M, N, F).transpose(1, 0, 2)
    assert rel_err(a.cpu().numpy(), ref1) < 2e-6
    Fout = 12
    Wk = (rng.standard_normal((F * K, Fout)) * orc.default_kernel_stddev(F, K)).astype(np.float32)
    bias = rng.standard_normal(Fout).astype(np.float32)
    fwd = orc.chebyshev_forward if basis == "chebyshev" else orc.monomial_forward
    B = {"chebyshev": _native.BASIS_CHEBYSHEV, "monomial": _native.BASIS_MONOMIAL}[basis]
    y, _ = _native.cheb_forward(plan, xd, _dev(Wk), _dev(bias), K, act=_native.ACT_RELU, precision=_native.PREC_BF16X6, basis=B)
    yp, _ = _native.cheb_forward(plain, xd, _dev(Wk), _dev(bias), K, act=_native.ACT_RELU, precision=_native.PREC_BF16X6, basis=B)
    assert rel_err(y.cpu().numpy(), fwd(Lt, x, Wk, K, bias=bias, activation="relu")) < 2e-6
    assert rel_err(y.cpu().numpy(), yp.cpu().numpy()) < 2e-6
    if basis == "chebyshev":
        dy = rng.standard_normal((N, M, Fout)).astype(np.float32)
        dw, _ = _native.cheb_backward_weights(plan, xd, _dev(dy), K)
        _, dW_ref = orc.chebyshev_backward(Lt, x, Wk, K, dy)
        assert rel_err(dw.cpu().numpy(), dW_ref) < 1e-5


def test_quick_start_model_values():
    """The reference's quick-start network (examples/quick_start.ipynb:118-127, 142-147): HealpyGCNN(n_neighbors=20) of four
    HealpyChebyshev(K=10, Fout=5 | 2, use_bias, use_bn, relu) layers with HealpyPool(p=1) between them, one input channel --
    20-neighbour graphs (ELL width 23), K = 10, channel counts that are no multiple of four: every step on the tiled kernel's
    scalar path, every contraction on the direct-operand kernel.  Values against the same walk with the float64 oracle layers
    (batch norm in inference mode at its initial statistics)."""
    from deepsphere import healpy_layers, healpy_networks

    nside = 16
    indices = np.arange(12 * nside * nside)
    layers = [healpy_layers.HealpyChebyshev(K=10, Fout=5, use_bias=True, use_bn=True, activation="relu"),
              healpy_layers.HealpyPool(p=1),
              healpy_layers.HealpyChebyshev(K=10, Fout=5, use_bias=True, use_bn=True, activation="relu"),
              healpy_layers.HealpyPool(p=1),
              healpy_layers.HealpyChebyshev(K=10, Fout=2)]
    torch.manual_seed(11)
    model = healpy_networks.HealpyGCNN(nside=nside, indices=indices, layers=layers, n_neighbors=20).cuda()
    model.eval()
    rng = np.random.default_rng(18)
    x = rng.standard_normal((4, len(indices), 1)).astype(np.float32)
    with torch.no_grad():
        y = model(_dev(x)).cpu().numpy()
    cur, cur_nside, cur_idx = x.astype(np.float64), nside, np.asarray(indices)
    for spec, mod in zip(layers, model):
        if isinstance(spec, healpy_layers.HealpyPool):
            cur = orc.healpy_pool(cur, spec.p, spec.pool_type)
            cur_idx = np.unique(cur_idx // 4 ** spec.p)
            cur_nside //= 2 ** spec.p
            continue
        L = healpix.healpix_laplacian(cur_nside, indices=cur_idx, n_neighbors=20, mode="knn")
        assert utils.csr_to_ell(L)[0].shape[1] > 12, "a 20-neighbour graph is wider than the fused kernels' templates"
        Lt, _ = orc.prepare_L(L)
        Wk = mod.kernel.detach().cpu().numpy().astype(np.float64)
        b = mod.bias.detach().cpu().numpy().reshape(-1).astype(np.float64) if mod.use_bias else None
        Fo = Wk.shape[1]
        cur = orc.chebyshev_forward(Lt, cur, Wk, spec.K, bias=b, activation=spec.activation,
                                    bn=(np.zeros(Fo), np.ones(Fo)) if spec.use_bn else None)
    assert y.shape == cur.shape == (4, len(indices) // 16, 2)
    err = rel_err(y, cur)
    print(f"quick-start model vs oracle composition: rel err {err:.2e}")
    assert err < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# Layers with more than 64 input channels: fused too (the BFS-tile kernel reads its weight fragments from global memory
# when those of all slices do not fit the LDS beside the planes)
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("prec,tol", [("fp32", 2e-6), ("bf16x6", 2e-6), ("bf16x3", TOL)])
@pytest.mark.parametrize("graph,nside,N,Fin,Fout,K", [
    ("grid", 64, 2, 128, 128, 5),   # a wide layer of the networks: structured tiles + class-G tiles, two 64-column blocks
    ("grid", 32, 1, 96, 40, 5),     # six slices, a ragged block
    ("knn", 32, 2, 128, 64, 4),     # every tile on the BFS-tile kernel
    ("grid", 32, 1, 256, 32, 3),    # sixteen slices
])
def test_wide_input_layers_run_fused(graph, nside, N, Fin, Fout, K, prec, tol):
    import bench

    if graph == "grid":
        cols, vals = _grid_ell(nside)
    else:
        cols, vals, _ = bench.build_laplacian_knn(nside, torch.device("cuda", 0), 8)
    M = cols.shape[0]
    plan = _native.LaplacianPlan(cols, vals, device=0)
    assert plan.fused_ok(Fin, Fout, K), "more than 64 input channels no longer fall back to the unfused path"
    rng = np.random.default_rng(Fin + Fout)
    x = rng.standard_normal((N, M, Fin)).astype(np.float32)
    W = (rng.standard_normal((Fin * K, Fout)) * orc.default_kernel_stddev(Fin, K)).astype(np.float32)
    b = rng.standard_normal(Fout).astype(np.float32)
    ref = orc.chebyshev_forward(_csr(cols, vals), x, W, K, bias=b, activation="relu")
    P = {"fp32": _native.PREC_FP32, "bf16x3": _native.PREC_BF16X3, "bf16x6": _native.PREC_BF16X6}[prec]
    y, ws = _native.cheb_forward(plan, _dev(x), _dev(W), _dev(b), K, act=_native.ACT_RELU, precision=P, algo=_native.ALGO_FUSED)
    err = rel_err(y.cpu().numpy(), ref)
    print(f"wide {graph} nside={nside} {Fin}->{Fout} K={K} {prec}: err {err:.2e}, tiles {plan.tile_counts(K)}")
    assert err < tol
    yu, _ = _native.cheb_forward(plan, _dev(x), _dev(W), _dev(b), K, act=_native.ACT_RELU, precision=P, algo=_native.ALGO_UNFUSED)
    assert rel_err(y.cpu().numpy(), yu.cpu().numpy()) < 2 * tol


# ---------------------------------------------------------------------------------------------------------------------
# First layers on the reference's own graphs (k-NN: a third of the tiles are class G): four maps per item in the BFS-tile kernel
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("prec,tol", [("fp32", 2e-6), ("bf16x6", 2e-6), ("bf16x3", 2 * TOL)])
@pytest.mark.parametrize("graph,nside,N,Fin,Fout,K,act", [
    ("knn", 64, 5, 1, 16, 5, "relu"),     # 1 -> 16 on the k-NN graph, a batch that ends inside a group of four
    ("knn", 32, 3, 4, 8, 5, None),        # the reference's test network shape
    ("knn", 32, 1, 3, 12, 4, "elu"),      # a single map, padded channels, deferred activation
    ("bfs", 32, 8, 2, 16, 3, "tanh"),     # the grid with the structured kernels switched off: every tile packed
    ("knn", 32, 6, 4, 20, 5, None),       # 20 columns: NOT packed (the ordinary path, for contrast)
    ("knn", 32, 3, 8, 8, 5, "relu"),      # 8 -> 8 (the reference's test network): two maps per item, one left over
    ("bfs", 32, 5, 6, 32, 4, None),       # six channels padded to eight, 32 columns, K = 4
    ("knn", 64, 4, 8, 24, 3, "elu"),      # two full groups
    ("knn", 32, 3, 5, 5, 5, "relu"),      # the quick-start model's 5 -> 5: padded to eight channels, a width that is no multiple of four
    ("bfs", 32, 6, 1, 5, 3, None),        # 1 -> 5 (its first layer): four maps per item, scalar stores, six maps = a group and a half
    ("grid", 32, 5, 2, 7, 4, "tanh"),     # the structured tiles of the grid with scalar stores
])
def test_bfs_tiles_pack_four_maps_for_narrow_layers(graph, nside, N, Fin, Fout, K, act, prec, tol):
    import bench

    opts = None
    if graph == "knn":
        cols, vals, _ = bench.build_laplacian_knn(nside, torch.device("cuda", 0), 8)
    else:
        cols, vals = _grid_ell(nside)
        opts = {_native.OPT_STRUCT: 0} if graph == "bfs" else None
    M = cols.shape[0]
    plan = _native.LaplacianPlan(cols, vals, device=0, options=opts)
    n_struct, n_bfs = plan.tile_counts(K)
    assert n_bfs > 0
    rng = np.random.default_rng(N + Fin + Fout)
    x = rng.standard_normal((N, M, Fin)).astype(np.float32)
    W = (rng.standard_normal((Fin * K, Fout)) * orc.default_kernel_stddev(Fin, K)).astype(np.float32)
    b = rng.standard_normal(Fout).astype(np.float32)
    ref = orc.chebyshev_forward(_csr(cols, vals), x, W, K, bias=b, activation=act)
    P = {"fp32": _native.PREC_FP32, "bf16x3": _native.PREC_BF16X3, "bf16x6": _native.PREC_BF16X6}[prec]
    A = {None: _native.ACT_NONE, "relu": _native.ACT_RELU, "elu": _native.ACT_ELU, "tanh": _native.ACT_TANH}[act]
    y, ws = _native.cheb_forward(plan, _dev(x), _dev(W), _dev(b), K, act=A, precision=P, algo=_native.ALGO_FUSED)
    err = rel_err(y.cpu().numpy(), ref)
    print(f"packed {graph} nside={nside} {Fin}->{Fout} K={K} N={N} {prec}: err {err:.2e}, tiles ({n_struct}, {n_bfs})")
    assert err < tol * (5 if act == "tanh" else 1)
    y2, _ = _native.cheb_forward(plan, _dev(x), _dev(W), _dev(b), K, act=A, precision=P, algo=_native.ALGO_FUSED, workspace=ws)
    assert torch.equal(y, y2)
    # a map's result does not depend on the group it shared a slice with (two maps: still a packed group; a single map runs
    # the plain form, equal to rounding)
    if N >= 2:
        y2m, _ = _native.cheb_forward(plan, _dev(x[N - 2:]), _dev(W), _dev(b), K, act=A, precision=P, algo=_native.ALGO_FUSED)
        assert torch.equal(y2m, y[N - 2:])
    y1, _ = _native.cheb_forward(plan, _dev(x[N - 1:]), _dev(W), _dev(b), K, act=A, precision=P, algo=_native.ALGO_FUSED)
    assert rel_err(y1[0].cpu().numpy(), y[N - 1].cpu().numpy()) < 2 * tol


def test_kept_weight_images_across_batch_classes():
    """A 1 -> 16 layer called with one map, then four, then one again: the tile kernels pack four maps into an item only when
    there is more than one, with another weight image -- the layer keys its kept images on the batch class."""
    nside, K = 64, 5
    cols, vals = _grid_ell(nside)
    M = cols.shape[0]
    layer = gnn_layers.Chebyshev.from_prepared_ell(cols, vals, K, Fout=16, device=torch.device("cuda", 0), use_bias=True, activation="relu")
    rng = np.random.default_rng(5)
    x = rng.standard_normal((4, M, 1)).astype(np.float32)
    with torch.no_grad():
        y1 = layer(_dev(x[:1])).clone()
        y4 = layer(_dev(x)).clone()
        y4b = layer(_dev(x)).clone()      # kept images, packed
        y1b = layer(_dev(x[:1])).clone()  # back to one map: re-packed for the plain form
        y1c = layer(_dev(x[:1])).clone()  # kept images, plain
    ref = orc.chebyshev_forward(_csr(cols, vals), x, layer.kernel.detach().cpu().numpy(), K,
                                bias=layer.bias.detach().cpu().numpy().reshape(-1), activation="relu")
    for y, r in ((y1, ref[:1]), (y4, ref), (y4b, ref), (y1b, ref[:1]), (y1c, ref[:1])):
        assert rel_err(y.cpu().numpy(), r) < 2e-6
    assert torch.equal(y4, y4b) and torch.equal(y1, y1b) and torch.equal(y1, y1c)


# ---------------------------------------------------------------------------------------------------------------------
# conv + HealpyPool(p = 1) in one forward (dsph_poly_forward_pool): the strip kernel of a first layer stores the pooled map
# ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("prec", ["fp32", "bf16x6", "bf16x3"])
@pytest.mark.parametrize("nside,N,Fin,Fout,K,basis,act,pool", [
    (128, 4, 1, 16, 5, "chebyshev", "relu", "MAX"),    # the first layer of the networks, pairs of maps
    (128, 3, 1, 16, 5, "chebyshev", "relu", "AVG"),    # the mean of the four children, an odd batch
    (128, 2, 2, 32, 4, "monomial", None, "MAX"),       # two channels, 32 columns, K = 4
    (256, 1, 1, 8, 3, "chebyshev", None, "AVG"),       # a single map, larger sphere (more row segments)
    (128, 2, 1, 64, 5, "chebyshev", "relu", "MAX"),    # two 32-column blocks
    (128, 3, 16, 32, 5, "chebyshev", "relu", "MAX"),   # the second layer of the networks: the eight-channel form
    (128, 2, 4, 8, 5, "chebyshev", None, "AVG"),       # 4 -> 8: the four-channel form with two maps per wave
    (128, 2, 8, 48, 4, "monomial", "relu", "MAX"),     # both halves of the four-channel form, two column blocks, K = 4 (an odd strip origin)
    (128, 1, 12, 16, 3, "chebyshev", None, "AVG"),     # twelve channels, K = 3
    (64, 4, 32, 64, 5, "chebyshev", "relu", "MAX"),    # 32 inputs: every structured tile pools in the structured kernel's store
    (64, 2, 64, 128, 5, "chebyshev", "relu", "AVG"),   # two 64-column blocks, four slices (a map too small for the Clenshaw strips)
    (32, 3, 4, 8, 5, "monomial", None, "MAX"),         # packed maps (four to an item) with the pooled store, no strips at all
    (128, 2, 1, 96, 5, "chebyshev", "relu", "MAX"),    # a first layer with three 32-column blocks over two 64-column launches
    (16, 3, 32, 32, 8, "chebyshev", "relu", "MAX"),    # K = 8: every tile on the BFS-tile kernel, which pools in its store too
    (8, 5, 128, 64, 5, "chebyshev", None, "AVG"),      # three tiles, eight slices read from global memory, the batch split over workgroups
])
def test_conv_and_pool_in_one_forward(nside, N, Fin, Fout, K, basis, act, pool, prec):
    cols, vals = _grid_ell(nside)
    M = cols.shape[0]
    plan = _native.LaplacianPlan(cols, vals, device=0)
    A = {None: _native.ACT_NONE, "relu": _native.ACT_RELU}[act]
    assert _native.pool_fusable(plan, N, Fin, Fout, K, A)
    assert not _native.pool_fusable(plan, N, Fin, Fout + 1, K, A), "pooled stores are 16 bytes wide"
    assert not _native.pool_fusable(plan, N, Fin, Fout, K, _native.ACT_TANH), "deferred activations run before the pooling"
    rng = np.random.default_rng(nside + Fout + K)
    x = rng.standard_normal((N, M, Fin)).astype(np.float32)
    W = (rng.standard_normal((Fin * K, Fout)) * orc.default_kernel_stddev(Fin, K)).astype(np.float32)
    b = rng.standard_normal(Fout).astype(np.float32)
    P = {"fp32": _native.PREC_FP32, "bf16x3": _native.PREC_BF16X3, "bf16x6": _native.PREC_BF16X6}[prec]
    B = {"chebyshev": _native.BASIS_CHEBYSHEV, "monomial": _native.BASIS_MONOMIAL}[basis]
    T = _native.POOL_MAX if pool == "MAX" else _native.POOL_AVG
    yp, ws = _native.cheb_forward_pool(plan, _dev(x), _dev(W), _dev(b), K, pool_type=T, act=A, precision=P, basis=B)
    # the two calls it replaces: bit for bit (same forward kernels, same order of the four children)
    y, _ = _native.cheb_forward(plan, _dev(x), _dev(W), _dev(b), K, act=A, precision=P, algo=_native.ALGO_FUSED, basis=B)
    y_ref = _native.healpix_pool(y, 4, T)
    assert torch.equal(yp, y_ref), f"max |diff| {float((yp - y_ref).abs().max()):.3e}"
    # and against the oracle
    fwd = orc.chebyshev_forward if basis == "chebyshev" else orc.monomial_forward
    ref = orc.healpy_pool(fwd(_csr(cols, vals), x, W, K, bias=b, activation=act), 1, pool)
    tol = 2e-6 if prec != "bf16x3" else 2 * TOL
    assert rel_err(yp.cpu().numpy(), ref) < tol
    yp2, _ = _native.cheb_forward_pool(plan, _dev(x), _dev(W), _dev(b), K, pool_type=T, act=A, precision=P, basis=B, workspace=ws,
                                       keep_weights=True)
    assert torch.equal(yp, yp2)


@pytest.mark.parametrize("pool_type", ["MAX"])
def test_model_fuses_a_first_layer_with_its_pooling(pool_type):
    """HealpyGCNN (8-neighbour k-NN graphs, the reference's default) in inference: Chebyshev(1 -> 16, bias, ReLU) + HealpyPool(p=1)
    run as one pass (Chebyshev.forward_pool), the later layers -- more input channels, or another activation -- as two; the
    output equals the layer-by-layer walk bit for bit, and the float64 oracle composition to tolerance."""
    from deepsphere import healpy_layers, healpy_networks

    nside = 128  # (from here on a map has strip rectangles: below, every tile is on the tile kernels and nothing is fused)
    indices = np.arange(12 * nside * nside)
    layers = [healpy_layers.HealpyChebyshev(K=5, Fout=16, use_bias=True, activation="relu"),
              healpy_layers.HealpyPool(p=1, pool_type=pool_type),
              healpy_layers.HealpyChebyshev(K=5, Fout=8, use_bias=True, activation="elu"),
              healpy_layers.HealpyPool(p=1, pool_type=pool_type)]
    torch.manual_seed(3)
    model = healpy_networks.HealpyGCNN(nside=nside, indices=indices, layers=layers, n_neighbors=8).cuda()
    model.eval()
    rng = np.random.default_rng(4)
    x = _dev(rng.standard_normal((3, len(indices), 1)).astype(np.float32))
    mods = list(model)
    with torch.no_grad():
        assert mods[0].forward_pool(x, pool_type) is not None, "the first layer has the fused pooling"
        assert mods[2].forward_pool(torch.zeros((3, len(indices) // 4, 16), device="cuda"), pool_type) is None
        y = model(x)
        cur = x
        for m in mods:
            cur = m(cur)
    assert torch.equal(y, cur)
    # the oracle composition
    ref, cur_nside, cur_idx = x.cpu().numpy().astype(np.float64), nside, np.asarray(indices)
    for spec, mod in zip(layers, mods):
        if isinstance(spec, healpy_layers.HealpyPool):
            ref = orc.healpy_pool(ref, spec.p, spec.pool_type)
            cur_idx = np.unique(cur_idx // 4)
            cur_nside //= 2
            continue
        Lt, _ = orc.prepare_L(mod.L)  # (the graph the model built: the 8-neighbour k-NN Laplacian of this resolution)
        Wk = mod.kernel.detach().cpu().numpy().astype(np.float64)
        b = mod.bias.detach().cpu().numpy().reshape(-1).astype(np.float64) if mod.use_bias else None
        ref = orc.chebyshev_forward(Lt, ref, Wk, spec.K, bias=b, activation=spec.activation)
    assert rel_err(y.cpu().numpy(), ref) < 1e-5
    # with autograd on the model takes the two layers (the fused pass has no backward)
    xg = x.clone().requires_grad_(True)
    assert mods[0].forward_pool(xg, pool_type) is None
