"""The Chebyshev family's pointer and workspace contract (include/dsphere.h, DESIGN.md "Alignment audit of the Chebyshev family"),
route by route: dsph_poly_forward_ex / _pool, dsph_cheb_planes, dsph_cheb_step, dsph_cheb_contract, dsph_cheb_backward_weights and
dsph_cheb_wgrad with x, y, w, bias, dy, dw, the planes and prev pushed 4 and 8 bytes off 16-byte alignment.

Every run (``_run``): inputs through ``helpers.offset_view`` and checksummed, outputs in ``large_map_ref.Guarded`` views pre-filled
with NaN, the workspace in a Guarded view of exactly the bytes the size query returns.  Afterwards both bands of every guarded
tensor are untouched, the output is finite everywhere, the inputs are unchanged and the values hold against the float64 oracle of
tests/cheb_memory_ref.py at the tolerance of the route's own test.  What a moved pointer may change is stated by the audit and
asserted: nothing (bit equality with the aligned run), the route (bit equality with a STRIPS_NEVER plan, twice the tolerance to the
aligned run), or a refusal that names the pointer.  No variant here reaches a 16-byte access through a misaligned pointer: each one
ends in a scalar branch, a fall-back or a host refusal."""

import ctypes

import numpy as np
import pytest
import torch
from scipy import sparse

import cheb_memory_ref as R
from deepsphere import _native, gnn_layers, healpix, healpy_layers
from helpers import offset_view, rel_err
from large_map_ref import Guarded, checksum
from oracle import cheb_oracle as orc

pytestmark = pytest.mark.gpu

PREC = {"fp32": _native.PREC_FP32, "bf16x3": _native.PREC_BF16X3, "bf16x6": _native.PREC_BF16X6}
ALGO = {"auto": _native.ALGO_AUTO, "fused": _native.ALGO_FUSED, "unfused": _native.ALGO_UNFUSED}
BASIS = {"chebyshev": _native.BASIS_CHEBYSHEV, "monomial": _native.BASIS_MONOMIAL}
ACT = {None: _native.ACT_NONE, "relu": _native.ACT_RELU, "elu": _native.ACT_ELU, "tanh": _native.ACT_TANH}

_plans, _refs, _runs = {}, {}, {}


def _plan(case, opts=None):
    """The case's plan (``opts``: other plan options than the table's), one per (graph, options)."""
    opts = case.opts if opts is None else tuple(opts)
    key = (case.graph, opts)
    if key not in _plans:
        g = R.graph(case.graph)
        _plans[key] = _native.LaplacianPlan(g["cols"], g["vals"], n_cols=g["n_cols"], device=0, levels=g["levels"],
                                            options={getattr(_native, k): getattr(_native, v) for k, v in opts})
    return _plans[key]


def _never(case):
    """The case's plan with the strip kernels switched off: what a forward runs on when y or bias bars the strips."""
    return tuple((k, v) for k, v in case.opts if k != "OPT_STRIPS") + R.NEVER


def _ref_dev(name):
    if name not in _refs:
        _refs[name] = torch.as_tensor(R.data(name)["ref"], dtype=torch.float64).cuda()
    return _refs[name]


def _err(got, ref):
    return float((got.to(torch.float64) - ref).abs().max()) / float(ref.abs().max())


def _ws(need):
    """The workspace as a guarded view of exactly ``need`` bytes rounded up to four, 16-byte aligned; None when nothing is needed."""
    return Guarded(((int(need) + 3) // 4,), "cuda") if need > 0 else None


def _assert_route(case, plan):
    prec = PREC[case.prec]
    if case.route == "unfused":
        assert case.algo == "unfused" or not plan.fused_ok(case.Fin, case.Fout, case.K), "the plan would run this shape fused"
        return
    if case.route == "chain":
        assert plan.uses_chain(case.Fin, case.Fout, case.K)
        return
    if case.kind in ("planes", "wgrad") and case.route == "bfs":
        return  # (their full breadth-first tables are not what tile_counts reports: ALGO_FUSED raises where they do not exist)
    n_struct, n_bfs = plan.tile_counts(case.K)
    n_strip = plan.strip_tiles(case.Fin, min(case.Fout, 64) if case.kind == "wgrad" else case.Fout, case.K, prec, N=case.N)
    if case.route == "bfs":
        assert n_struct == 0 and n_bfs > 0 and n_strip == 0
    elif case.route == "struct":
        assert n_struct > 0 and (n_strip == 0 or case.kind == "parts")
    else:
        assert n_strip > 0, "the strip kernel this case is about takes no tile"


def _run(name, off=None, opts=None, algo=None, part=None, into=None):
    """One guarded run of case ``name`` with the pointers of ``off`` (x, y, w, bias, dy, dw: floats off 16-byte alignment):
    -> the output as a tensor of its own.  ``into``: (Guarded out, Guarded workspace) of an earlier part of the same forward."""
    off = off or {}
    d = R.data(name)
    case, g = d["case"], d["graph"]
    plan = _plan(case, opts)
    if opts is None:
        _assert_route(case, plan)
    prec, alg = PREC[case.prec], ALGO[case.algo if algo is None else algo]
    N, Fin, Fout, K = case.N, case.Fin, case.Fout, case.K
    ins = {"x": offset_view(d["x"], off.get("x", 0))}
    for k in ("w", "bias", "dy"):
        if d[k] is not None:
            ins[k] = offset_view(d[k], off.get(k, 0))
    sums = {k: checksum(t) for k, t in ins.items()}
    if case.kind == "wgrad":
        need = int(_native.lib().dsph_backward_weights_workspace_bytes(plan.handle, N, Fin, Fout, K, alg))
    else:
        need = 0 if case.kind == "planes" else plan.workspace_bytes(N, Fin, Fout, K, prec, _native.ALGO_FUSED if case.kind == "pool" else alg)
    if into is not None:
        out, ws = into
    else:
        out, ws = Guarded(R.out_shape(case, g), "cuda", off.get("dw" if case.kind == "wgrad" else "y", 0)), _ws(need)
    wsv = None if ws is None else ws.view
    kw = dict(basis=BASIS[case.basis])
    if case.kind in ("forward", "parts"):
        _, w2 = _native.cheb_forward(plan, ins["x"], ins["w"], ins.get("bias"), K, act=ACT[case.act], precision=prec, algo=alg, workspace=wsv,
                                     out=out.view, part=_native.PART_ALL if part is None else part, **kw)
    elif case.kind == "pool":
        _, w2 = _native.cheb_forward_pool(plan, ins["x"], ins["w"], ins.get("bias"), K, pool_type=_native.POOL_MAX, act=ACT[case.act],
                                          precision=prec, workspace=wsv, out=out.view, **kw)
    elif case.kind == "planes":
        planes, w2 = _native.cheb_planes(plan, ins["x"], K, algo=alg, out=out.view, **kw), None
        assert planes[0] is ins["x"] and all(planes[k + 1].data_ptr() == out.view[k].data_ptr() for k in range(K - 1))
    else:
        _, w2 = _native.cheb_backward_weights(plan, ins["x"], ins["dy"], K, algo=alg, workspace=wsv, precision=prec, out=out.view, **kw)
    torch.cuda.synchronize()
    assert w2 is wsv or (case.kind == "wgrad" and need == 0), "the wrapper replaced a workspace of the size the query asked for"
    out.check(f"{name} {off}: output")
    if ws is not None:
        ws.check(f"{name} {off}: workspace of {need} bytes")
    for k, t in ins.items():
        assert checksum(t) == sums[k], f"{name} {off}: {k} was written to"
    if part is None:
        assert bool(torch.isfinite(out.view).all()), f"{name} {off}: an element of the output was never written"
        err = _err(out.view, _ref_dev(name))
        print(f"{name} {off or 'aligned'} opts={opts} algo={algo}: rel err {err:.2e} (tolerance {R.tolerance(case):.0e}), workspace {need} bytes")
        assert err < R.tolerance(case)
    return out.view.clone()


def _base(name, opts=None, algo=None):
    """The aligned run of a case (on its own plan, or with other options / another algo), computed once."""
    key = (name, opts, algo)
    if key not in _runs:
        _runs[key] = _run(name, None, opts, algo)
    return _runs[key]


def _close(name, a, b, factor=2):
    case = R.BY_NAME[name]
    d = float((a - b).abs().max()) / float(_ref_dev(name).abs().max())
    assert d < factor * R.tolerance(case), f"{name}: {d:.2e} between the two routes"


FORWARD = [c.name for c in R.CASES if c.kind == "forward"]
WGRAD = [c.name for c in R.CASES if c.kind == "wgrad"]
PLANES = [c.name for c in R.CASES if c.kind == "planes"]


@pytest.mark.parametrize("name", FORWARD + WGRAD + PLANES + ["pool_4_8_5"])
def test_aligned_run_keeps_to_its_buffers(name):
    """Every route on aligned pointers: bands of the output and of a workspace of exactly the queried size, NaN pre-fill gone,
    inputs unchanged, values against the oracle; a second run agrees bit for bit."""
    a = _base(name)
    assert torch.equal(a, _run(name))


@pytest.mark.parametrize("name", FORWARD + WGRAD + ["pool_4_8_5"])
def test_x_off_alignment_changes_no_bit(name):
    """x four bytes off.  Fused routes: the wrapper hands the kernels an aligned copy (_native._fused_x; Fin % 4 != 0: the kernels read
    the padded copy that fused_pad_kernel, cheb_fused.hip, makes by the element) -- same kernels, same bits.  Unfused routes: the step
    kernels' scalar form (cheb_step.hip launch_cheb_step's vec4, cheb_tstep.hip's VEC) and the contraction's (cheb_tcontract.hip
    vec_in) change the width of the loads, not the order of a row's additions; cheb_wgrad.hip reads by the element anyway."""
    assert torch.equal(_run(name, {"x": 1}), _base(name))


@pytest.mark.parametrize("name", FORWARD + ["pool_4_8_5"])
def test_w_off_alignment_changes_no_bit(name):
    """w four bytes off: every weight-preparation kernel (fused_wprep_kernel, struct_ / strip_ / qstrip_ / qstrip8_ / istrip_wprep_kernel,
    split_weights_kernel) and cheb_tcontract.hip's wf_gather read w by the element: same route, same bits."""
    assert torch.equal(_run(name, {"w": 1}), _base(name))


@pytest.mark.parametrize("name", FORWARD + ["pool_4_8_5"])
def test_bias_off_alignment(name):
    """bias four bytes off.  Only the two quad-strip kernels load bias in 16-byte pieces (cheb_qstrip_kernel.h, cheb_qstrip8_kernel.h:
    `bv = *reinterpret_cast<const qs_f4*>(a.bias + ...)`): make_route (cheb_fused.hip) keeps their tiles on the tile kernels then, whose
    bits a STRIPS_NEVER plan shows.  Everywhere else bias is read by the element into the LDS: same route, same bits."""
    case = R.BY_NAME[name]
    got = _run(name, {"bias": 1})
    if case.bias_off == "same":
        assert torch.equal(got, _base(name))
    else:
        assert torch.equal(got, _base(name, _never(case))), "a misaligned bias keeps the quad strips' tiles on the tile kernels"
        _close(name, got, _base(name))


@pytest.mark.parametrize("floats", [1, 2])
@pytest.mark.parametrize("name", FORWARD)
def test_y_off_alignment(name, floats):
    """y four and eight bytes off.  "same": the BFS-tile and structured-tile kernels store by the element (vec_ok, cheb_fused_kernel.h /
    cheb_struct_kernel.h), cheb_tcontract.hip does when Fout % 4 != 0.  "tiles": make_route hands the strips' tiles to the tile
    kernels -- the bits of a STRIPS_NEVER plan, twice the tolerance to the strips' own.  "close": another kernel takes over
    (cheb_tcontract.hip returns false for Fout % 4 == 0, cheb_contract.hip's exact-fp32 kernels run; the chain's last pass
    loses its strips)."""
    case = R.BY_NAME[name]
    got = _run(name, {"y": floats})
    if case.y_off == "same":
        assert torch.equal(got, _base(name))
    elif case.y_off == "tiles":
        assert torch.equal(got, _base(name, _never(case))), "a misaligned y keeps the strips' tiles on the tile kernels"
        _close(name, got, _base(name))
    else:
        _close(name, got, _base(name))


@pytest.mark.parametrize("name", WGRAD)
def test_dy_and_dw_off_alignment_change_no_bit(name):
    """dy, then dw, four bytes off.  The BFS-tile kernel's weight-gradient mode and cheb_wgrad.hip read dy by the element; the
    quad-strip gradient reads it in 16-byte pieces (cheb_qwgrad_kernel.h) and the wrapper hands it an aligned copy.  dw is written by
    the reduction kernels, by the element."""
    assert torch.equal(_run(name, {"dy": 1}), _base(name))
    assert torch.equal(_run(name, {"dw": 1}), _base(name))


def test_quad_strip_gradient_really_runs_and_falls_back_on_a_misaligned_dy():
    """The quad-strip weight gradient through the C ABI itself: with dy four bytes off dsph_cheb_backward_weights runs the BFS-tile
    kernel on every tile (what a plan without strips does: its bits), in a workspace of the same size; with x four bytes off it
    refuses, naming x, before anything is launched."""
    name = "wgrad_quad_64_64_5"
    d = R.data(name)
    case = d["case"]
    plan = _plan(case)
    quad, plain = _base(name), _base(name, _never(case))
    assert not torch.equal(quad, plain), "the two plans run different kernels (else this test exercises nothing)"
    need = int(_native.lib().dsph_backward_weights_workspace_bytes(plan.handle, case.N, case.Fin, case.Fout, case.K, _native.ALGO_FUSED))

    def raw(x, dy, dw, ws):
        return _native.lib().dsph_cheb_backward_weights(plan.handle, _native._ptr(x), _native._ptr(dy), _native._ptr(dw.view), case.N, case.Fin,
                                                        case.Fout, case.K, BASIS[case.basis], PREC[case.prec], _native.ALGO_FUSED,
                                                        _native._ptr(ws.view), need, _native._stream_ptr(x.device))

    x, dy, dw, ws = offset_view(d["x"], 0), offset_view(d["dy"], 1), Guarded(quad.shape, "cuda"), _ws(need)
    assert raw(x, dy, dw, ws) == _native.OK, _native.last_error()
    torch.cuda.synchronize()
    dw.check("dw")
    ws.check("workspace")
    assert torch.equal(dw.view, plain)
    assert _err(dw.view, _ref_dev(name)) < R.tolerance(case)
    x1, dw1 = offset_view(d["x"], 1), Guarded(quad.shape, "cuda")
    assert raw(x1, offset_view(d["dy"], 0), dw1, ws) == -1
    assert "x must be 16-byte aligned" in _native.last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(dw1.view).all()), "a refusal launches nothing"


@pytest.mark.parametrize("name", PLANES)
def test_planes_off_alignment(name):
    """dsph_cheb_planes: ALGO_AUTO with x or the planes off alignment takes the step kernels (no workspace depends on the route: the
    C ABI's own choice) -- the unfused run's bits; ALGO_FUSED with x off runs on the wrapper's aligned copy, bit-equal to the aligned
    run, and refuses misaligned planes by name."""
    fused, unfused = _base(name, algo="fused"), _base(name, algo="unfused")
    assert torch.equal(_base(name), fused), "ALGO_AUTO runs the fused planes mode on aligned pointers"
    _close(name, fused, unfused)
    for off in ({"x": 1}, {"y": 1}, {"y": 2}):
        assert torch.equal(_run(name, off), unfused), f"ALGO_AUTO with {off} runs on the step kernels"
    assert torch.equal(_run(name, {"x": 1}, algo="fused"), fused)
    assert torch.equal(_run(name, {"x": 1}, algo="unfused"), unfused)
    with pytest.raises(ValueError, match="planes must be 16-byte aligned"):
        _run(name, {"y": 1}, algo="fused")


def test_pool_refuses_a_misaligned_pooled_map_by_name():
    """dsph_poly_forward_pool stores the pooled map in 16-byte pieces in every kernel: a y_pooled off alignment is refused, and the
    message says which pointer it was."""
    with pytest.raises(ValueError, match="y_pooled must be 16-byte aligned"):
        _run("pool_4_8_5", {"y": 1})


def test_c_abi_refuses_a_misaligned_x_and_workspace_by_name():
    """The C ABI itself (no wrapper in between) on a fused route: x four bytes off with Fin % 4 == 0, then the workspace four bytes off,
    are refused with DSPH_E_BADARG before any launch -- y keeps its NaN pre-fill -- and the message names the pointer; with
    DSPH_ALGO_UNFUSED the same x runs."""
    name = "bfs_16_32_5"
    d = R.data(name)
    case = d["case"]
    plan = _plan(case)
    need = plan.workspace_bytes(case.N, case.Fin, case.Fout, case.K, PREC[case.prec], _native.ALGO_FUSED)
    w, b = offset_view(d["w"], 0), offset_view(d["bias"], 0)

    def raw(x, y, ws_ptr, ws_bytes, algo):
        return _native.lib().dsph_poly_forward_ex(plan.handle, _native._ptr(x), _native._ptr(w), _native._ptr(b), _native._ptr(y.view), case.N,
                                                  case.Fin, case.Fout, case.K, BASIS[case.basis], ACT[case.act], PREC[case.prec], algo,
                                                  _native.PART_ALL, 0, ws_ptr, ws_bytes, _native._stream_ptr(x.device))

    ws = Guarded(((need + 3) // 4 + 1,), "cuda")
    y = Guarded(R.out_shape(case), "cuda")
    assert raw(offset_view(d["x"], 1), y, _native._ptr(ws.view), need, _native.ALGO_FUSED) == -1
    assert "x must be 16-byte aligned" in _native.last_error()
    assert raw(offset_view(d["x"], 1), y, _native._ptr(ws.view), need, _native.ALGO_AUTO) == -1, "AUTO resolves to the fused route from plan and shape"
    assert "x must be 16-byte aligned" in _native.last_error()
    assert raw(offset_view(d["x"], 0), y, ctypes.c_void_p(ws.view.data_ptr() + 4), need, _native.ALGO_FUSED) == -1
    assert "workspace must be 16-byte aligned" in _native.last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.view).all()) and bool(torch.isnan(ws.view).all()), "a refusal launches nothing"
    need_u = plan.workspace_bytes(case.N, case.Fin, case.Fout, case.K, PREC[case.prec], _native.ALGO_UNFUSED)
    wsu = _ws(need_u)
    assert raw(offset_view(d["x"], 1), y, _native._ptr(wsu.view), need_u, _native.ALGO_UNFUSED) == _native.OK, _native.last_error()
    torch.cuda.synchronize()
    y.check()
    wsu.check()
    assert _err(y.view, _ref_dev(name)) < R.tolerance(case)


@pytest.mark.parametrize("off", [{}, {"x": 1}, {"y": 1}, {"y": 2}, {"w": 1}, {"bias": 1}], ids=str)
def test_parts_fill_only_their_own_rows(off):
    """Interior, then boundary, of a sharded plan into one guarded y: each part leaves the other's rows at their NaN pre-fill, both
    together fill the map, against the whole sphere's forward on the rank's rows."""
    name = "parts_16_32_5"
    d = R.data(name)
    case, g = d["case"], d["graph"]
    plan = _plan(case)
    need = plan.workspace_bytes(case.N, case.Fin, case.Fout, case.K, PREC[case.prec], _native.ALGO_FUSED)
    out, ws = Guarded(R.out_shape(case, g), "cuda", off.get("y", 0)), _ws(need)
    inner = _run(name, off, part=_native.PART_INTERIOR, into=(out, ws))
    wrote_inner = ~torch.isnan(inner)
    assert bool(wrote_inner.any()) and not bool(wrote_inner.all())
    out.view.fill_(float("nan"))
    outer = _run(name, off, part=_native.PART_BOUNDARY, into=(out, ws))
    wrote_outer = ~torch.isnan(outer)
    assert bool((wrote_inner ^ wrote_outer).all()), "the two parts write disjoint rows that cover the map"
    both = torch.where(wrote_inner, inner, outer)
    err = _err(both, _ref_dev(name))
    print(f"{name} {off or 'aligned'}: rel err {err:.2e}")
    assert err < R.tolerance(case)
    whole = _base(name)
    if "y" in off:
        _close(name, both, whole)  # (a misaligned y bars the input-side strips: another kernel on their tiles)
    else:
        assert torch.equal(both, whole)


# ---- the unfused entry points alone ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("graph,F", [(("knn", 8, 8), 8), (("knn", 8, 8), 7), (("knn", 16, 20), 4)], ids=["gather-8", "gather-7", "tiled-4"])
def test_step_alone_with_each_pointer_off(graph, F):
    """dsph_cheb_step (cheb_step.hip; the tiled kernel of cheb_tstep.hip on the wide graph) with in, prev and out in turn four bytes
    off: the launch's `vec4` / `vec` flag picks the scalar form, which adds a row's terms in the same order -- the aligned run's bits,
    2e-6 to out = 2 L~ in - prev in float64."""
    g = R.graph(graph)
    plan = _native.LaplacianPlan(g["cols"], g["vals"], device=0)
    M, N = g["cols"].shape[0], 2
    rng = np.random.default_rng(F)
    a, p = rng.standard_normal((N, M, F)).astype(np.float32), rng.standard_normal((N, M, F)).astype(np.float32)
    flat = lambda v: v.astype(np.float64).transpose(1, 0, 2).reshape(M, -1)  # noqa: E731
    ref = torch.as_tensor((2.0 * (g["Lt"] @ flat(a)) - flat(p)).reshape(M, N, F).transpose(1, 0, 2).copy()).cuda()
    outs = []
    for off in ({}, {"in": 1}, {"prev": 1}, {"out": 1}, {"out": 2}, {"in": 1, "prev": 2, "out": 3}):
        ta, tp = offset_view(a, off.get("in", 0)), offset_view(p, off.get("prev", 0))
        sa, sp = checksum(ta), checksum(tp)
        out = Guarded((N, M, F), "cuda", off.get("out", 0))
        _native.cheb_step(plan, ta, tp, 2.0, 1.0, out=out.view)
        torch.cuda.synchronize()
        out.check(f"step {off}")
        assert checksum(ta) == sa and checksum(tp) == sp
        assert bool(torch.isfinite(out.view).all())
        assert _err(out.view, ref) < 2e-6
        outs.append(out.view.clone())
    assert all(torch.equal(o, outs[0]) for o in outs[1:])


@pytest.mark.parametrize("prec,Fout", [("fp32", 12), ("bf16x3", 12), ("fp32", 70)])
def test_contract_alone_with_one_plane_off(prec, Fout):
    """dsph_cheb_contract on K planes of which one is four bytes off (cheb_tcontract.hip: vec_in covers every plane), then with y off
    as well (Fout % 4 == 0: the fall-back to cheb_contract.hip, vec_a / vec_ok; Fout = 70: the same kernel's scalar stores)."""
    d = R.data("wgrad_unfused_7_70_3" if Fout == 70 else "unfused_8_12_4")
    case, g = d["case"], d["graph"]
    N, M, Fin, K = case.N, g["cols"].shape[0], case.Fin, case.K
    planes = orc.chebyshev_planes(g["Lt"], d["x"], K).astype(np.float32)
    rng = np.random.default_rng(Fout)
    w = (rng.standard_normal((Fin * K, Fout)) * orc.default_kernel_stddev(Fin, K)).astype(np.float32)
    b = rng.standard_normal(Fout).astype(np.float32)
    ref = (planes.astype(np.float64).transpose(1, 2, 3, 0).reshape(N * M, Fin * K) @ w.astype(np.float64)).reshape(N, M, Fout) + b
    ref = torch.as_tensor(ref).cuda()
    tol = 2e-6 if prec == "fp32" else 2e-5  # (bf16x3 below 16 input channels)
    outs = {}
    for off in ({}, {"plane": 1}, {"plane": 1, "y": 1}, {"w": 1, "bias": 1}):
        pl = [offset_view(planes[k], off.get("plane", 0) if k == 1 else 0) for k in range(K)]
        tw, tb = offset_view(w, off.get("w", 0)), offset_view(b, off.get("bias", 0))
        sums = [checksum(t) for t in pl + [tw, tb]]
        out = Guarded((N, M, Fout), "cuda", off.get("y", 0))
        _native.cheb_contract(pl, tw, tb, M, K, precision=PREC[prec], out=out.view)
        torch.cuda.synchronize()
        out.check(f"contract {off}")
        assert [checksum(t) for t in pl + [tw, tb]] == sums
        assert bool(torch.isfinite(out.view).all())
        assert _err(out.view, ref) < tol
        outs[str(off)] = out.view.clone()
    base = outs["{}"]
    assert torch.equal(outs[str({"plane": 1})], base) and torch.equal(outs[str({"w": 1, "bias": 1})], base)
    if Fout % 4:
        assert torch.equal(outs[str({"plane": 1, "y": 1})], base)
    else:
        assert float((outs[str({"plane": 1, "y": 1})] - base).abs().max()) / float(ref.abs().max()) < 2 * tol


def test_wgrad_alone_on_an_odd_row_count():
    """dsph_cheb_wgrad (cheb_wgrad.hip) on M - 7 rows of planes of M rows -- an odd count, so the last trip of eight row pairs is
    ragged --, 7 channels and 70 columns, in a workspace of exactly dsph_wgrad_workspace_bytes: dw, a plane and dy in turn off."""
    d = R.data("wgrad_unfused_7_70_3")
    case, g = d["case"], d["graph"]
    N, M, Fin, Fout, K = case.N, g["cols"].shape[0], case.Fin, case.Fout, case.K
    rows = M - 7
    dy = np.ascontiguousarray(d["dy"][:, :rows])
    ref = np.ascontiguousarray(d["planes"].astype(np.float64)[:, :, :rows].transpose(3, 0, 1, 2)).reshape(Fin * K, -1) @ dy.astype(np.float64).reshape(-1, Fout)
    ref = torch.as_tensor(ref).cuda()
    need = int(_native.lib().dsph_wgrad_workspace_bytes(N, rows, Fin, Fout, K))
    outs = []
    for off in ({}, {"dw": 1}, {"plane": 1}, {"dy": 1}):
        pl = [offset_view(d["planes"][k], off.get("plane", 0) if k == 2 else 0) for k in range(K)]
        tdy = offset_view(dy, off.get("dy", 0))
        sums = [checksum(t) for t in pl + [tdy]]
        dw, ws = Guarded((Fin * K, Fout), "cuda", off.get("dw", 0)), _ws(need)
        _, w2 = _native.cheb_wgrad(pl, tdy, rows=rows, workspace=ws.view, out=dw.view)
        torch.cuda.synchronize()
        assert w2 is ws.view
        dw.check(f"wgrad {off}: dw")
        ws.check(f"wgrad {off}: workspace")
        assert [checksum(t) for t in pl + [tdy]] == sums
        assert bool(torch.isfinite(dw.view).all())
        assert _err(dw.view, ref) < 2e-5
        outs.append(dw.view.clone())
    assert all(torch.equal(o, outs[0]) for o in outs[1:])


# ---- the layers ------------------------------------------------------------------------------------------------------------------

class _MisalignedGradient(torch.autograd.Function):
    """Identity whose backward hands its gradient on as a view four bytes off 16-byte alignment."""

    @staticmethod
    def forward(ctx, y):
        return y.view_as(y)

    @staticmethod
    def backward(ctx, g):
        return offset_view(g, 1)


@pytest.mark.parametrize("where", ["gnn_layers", "healpy_layers"])
@pytest.mark.parametrize("activation", [None, "relu"])
def test_layers_take_x_and_dy_off_alignment(where, activation):
    """gnn_layers.Chebyshev and the layer a HealpyChebyshev spec builds, forward and backward, on a fused-capable plan with
    Fin = 16: x as a view four bytes off (the C ABI's fused route refuses such an x: the wrapper's aligned copy), and the gradient
    arriving as such a view.  Values against the oracle's closed forms as in test_layer_gradients_match_oracle."""
    rng = np.random.default_rng(5)
    L = healpix.healpix_laplacian(16, mode="knn")
    M, N, Fin, Fout, K = L.shape[0], 2, 16, 32, 5
    x_np = rng.standard_normal((N, M, Fin)).astype(np.float32)
    W_np = (rng.standard_normal((Fin * K, Fout)) * orc.default_kernel_stddev(Fin, K)).astype(np.float32)
    dy_np = rng.standard_normal((N, M, Fout)).astype(np.float32)
    init = lambda t: t.copy_(torch.from_numpy(W_np))  # noqa: E731
    with torch.enable_grad():
        if where == "gnn_layers":
            layer = gnn_layers.Chebyshev(L=L, K=K, Fout=Fout, use_bias=True, activation=activation, initializer=init)
        else:
            layer = healpy_layers.HealpyChebyshev(K, Fout=Fout, use_bias=True, activation=activation, initializer=init)._get_layer(L)
        layer.build((N, M, Fin))  # (the weights exist from here on: the bias is drawn at random, the oracle needs it before the backward)
        Lt = (sparse.csr_matrix(L, dtype=np.float64) * (1.5 / layer.lmax) - sparse.identity(M)).tocsr().astype(np.float32)  # the layer's own L~
        b = layer.bias.detach().cpu().numpy().reshape(-1)
        z = orc.chebyshev_forward(Lt, x_np, W_np, K, bias=b)
        if activation == "relu":
            # relu' is not defined to the arithmetic's accuracy where the pre-activation is zero to within the forward's rounding (a
            # hundred or so of these 2e5 elements lie within 1e-4 max|z| of zero, and lmax comes from ARPACK's random start): no
            # gradient arrives there, so the oracle's mask and the kernel's agree on every element that counts
            dy_np = dy_np * (np.abs(z) > 1e-4 * np.abs(z).max())
        x = offset_view(x_np, 1).requires_grad_(True)
        assert x.data_ptr() % 16 == 4
        y = _MisalignedGradient.apply(layer(x))
        y.backward(torch.as_tensor(dy_np, dtype=torch.float32).cuda())
    dz = dy_np * (z > 0) if activation == "relu" else dy_np
    dx_ref, dW_ref = orc.chebyshev_backward(Lt, x_np, W_np, K, dz)
    assert rel_err(y.detach().cpu().numpy(), orc.chebyshev_forward(Lt, x_np, W_np, K, bias=b, activation=activation)) < 2e-5
    assert rel_err(x.grad.cpu().numpy(), dx_ref) < 2e-5
    assert rel_err(layer.kernel.grad.cpu().numpy(), dW_ref) < 2e-5
    assert rel_err(layer.bias.grad.cpu().numpy().reshape(-1), dz.sum((0, 1))) < 2e-5
    # the inference forward (bias and activation in the kernel's epilogue) on the same view
    with torch.no_grad():
        yi = layer(offset_view(x_np, 1))
    assert rel_err(yi.cpu().numpy(), orc.chebyshev_forward(Lt, x_np, W_np, K, bias=b, activation=activation)) < 2e-5

