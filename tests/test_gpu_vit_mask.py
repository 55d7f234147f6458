"""GPU tests of the dense attention's ``mask`` argument -- the reference's ``mask * -1e9`` added to the logits inside the flash
kernels, in all three arithmetics -- and of the layers that carry it (``pytest -m gpu``).

Reference: tests/dense_attention_mask_ref.py (float64 after the float32 logit + mask sum).  Error measure: helpers.rel_err.  N = 2.

Tolerances: those of tests/test_gpu_vit.py and tests/test_gpu_vit_precision.py.  "fp32" and "bf16x6": 1e-5 on out and on both
parts of the statistic pair (m, log l), 2e-5 on dq, dk, dv.  "bf16x3": T + 3 E_emul, E_emul the error of the masked emulation of
the arithmetic on the same inputs against the same reference, computed here on the CPU; an emulation off by more than 1e-4 fails
the test rather than loosening the bound.  A 0/1 mask makes the softmax one over a subset of keys and a soft bias shifts logits by
O(1): the error model of those files carries over.  Layer tests: ten times the error the same computation shows in torch float32
on the CPU.

Sizes M = 2 (smallest map with non-zero dq), 64 (one exact tile), 65 (one key past a tile, odd: mask rows are unaligned), 331
(several tiles and a ragged tail).  fp32 shapes (heads, depth) = (1, 4), (3, 8), (4, 16), (2, 32), (1, 64): the code paths by
depth; split shapes (2, 32), (1, 64).
"""

import functools

import numpy as np
import pytest
import torch

import deepsphere
import dense_attention_mask_ref as mref
from deepsphere import _native, gnn_transformers, healpix
from deepsphere.healpy_layers import Healpy_ViT
from helpers import rel_err

pytestmark = pytest.mark.gpu

N = 2
SIZES = [2, 64, 65, 331]
CONFIGS = [("fp32", 1, 4), ("fp32", 3, 8), ("fp32", 4, 16), ("fp32", 2, 32), ("fp32", 1, 64),
           ("bf16x6", 2, 32), ("bf16x6", 1, 64), ("bf16x3", 2, 32), ("bf16x3", 1, 64)]
CODES = {"fp32": _native.PREC_FP32, "bf16x6": _native.PREC_BF16X6, "bf16x3": _native.PREC_BF16X3}
FORMS = ["key", "per_map", "per_head", "pair", "full"]
T_OUT, T_GRAD = 1e-5, 2e-5
EMUL_CAP = 1e-4
NAMES = ("out", "m", "log l", "dq", "dk", "dv")
TOLS = (T_OUT, T_OUT, T_OUT, T_GRAD, T_GRAD, T_GRAD)


def config_id(c):
    return f"{c[0]}-{c[1]}x{c[2]}"


@functools.lru_cache(maxsize=None)
def inputs(M, d):
    rng = np.random.default_rng(0)
    return tuple(rng.standard_normal((N, M, d)).astype(np.float32) for _ in range(4))  # q, k, v, g


def form_shape(form, M, heads):
    return {"key": (M,), "per_map": (N, 1, 1, M), "per_head": (1, heads, 1, M), "pair": (M, M), "full": (N, heads, M, M)}[form]


@functools.lru_cache(maxsize=None)
def build_mask(spec, M, heads):
    """spec = (form, kind[, extra]) -> float32 array of the form's shape, read-only.
    kinds: "binary" (about 30 % ones, every row of keys keeps a zero), "zeros", "soft" (b * 1e-9, b uniform in [0, 4]),
    "keys" (extra = (lo, hi): exactly the keys lo..hi-1 masked), "rows" (binary, rows 0 and M - 1 of a pair mask all ones)."""
    form, kind = spec[0], spec[1]
    shape = form_shape(form, M, heads)
    rng = np.random.default_rng(1234 + 7 * M + heads)
    if kind == "zeros":
        mask = np.zeros(shape, dtype=np.float32)
    elif kind == "soft":
        mask = (rng.uniform(0.0, 4.0, size=shape) * 1e-9).astype(np.float32)
    elif kind == "keys":
        mask = np.zeros(shape, dtype=np.float32)
        mask[..., spec[2][0]:spec[2][1]] = 1.0
    else:
        mask = (rng.uniform(size=shape) < 0.3).astype(np.float32)
        rows = mask.reshape(-1, M)
        for i in np.nonzero(rows.min(axis=1) > 0)[0]:  # a row of keys with no zero left: open one
            rows[i, rng.integers(M)] = 0.0
        # A softmax over ONE key has dq = dk = 0 exactly, and rel_err has no scale against a zero reference (at M = 2 any masked
        # key does that): the first row of keys keeps two, so that the reference gradients of a case are never all zero.
        rows[0, np.nonzero(rows[0])[0][:max(0, 2 - int((rows[0] == 0).sum()))]] = 0.0
        if kind == "rows":
            assert form == "pair"
            mask[0, :] = 1.0
            mask[M - 1, :] = 1.0
    mask.setflags(write=False)
    return mask


def assert_mask_condition(mask, M, on_purpose=()):
    """Apart from the query rows masked on purpose, every row keeps an unmasked key and at most half of the entries are masked."""
    mask4 = mask.reshape((1,) * (4 - mask.ndim) + mask.shape)
    full = np.broadcast_to(mask4, np.broadcast_shapes(mask4.shape, (1, 1, M, M)))
    keep = np.array([i for i in range(M) if i not in on_purpose], dtype=np.int64)
    if keep.size == 0:
        return
    rest = full[:, :, keep, :]
    assert (rest.min(axis=-1) == 0).all(), "a query row outside the purpose of the test has every key masked"
    assert (rest != 0).mean() <= 0.5, "more than half of the entries are masked"


@functools.lru_cache(maxsize=None)
def reference(M, heads, depth, spec):
    q, k, v, g = inputs(M, heads * depth)
    out, stat, dq, dk, dv = mref.attention(q, k, v, heads, build_mask(spec, M, heads), g)
    return out, stat[..., 0], stat[..., 1], dq, dk, dv


@functools.lru_cache(maxsize=None)
def emulation_errors(M, heads, depth, spec, precision):
    """E_emul per quantity of NAMES; 0 for "fp32" and "bf16x6", whose bounds take no allowance."""
    if precision != "bf16x3":
        return (0.0,) * 6
    q, k, v, g = inputs(M, heads * depth)
    out, stat, dq, dk, dv = mref.split_attention(q, k, v, heads, precision, build_mask(spec, M, heads), g)
    errs = tuple(rel_err(a, b) for a, b in zip((out, stat[..., 0], stat[..., 1], dq, dk, dv), reference(M, heads, depth, spec)))
    print(f"emulation {precision} M {M} {heads}x{depth} {spec}: " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= EMUL_CAP, f"the emulation itself is off by {errs}: it would loosen the bound"
    return errs


def run_native(M, heads, depth, precision, mask_t):
    """Forward and backward through the entry points: -> [out, m, log l, dq, dk, dv] as tensors on the device."""
    q, k, v, g = (torch.as_tensor(a).cuda() for a in inputs(M, heads * depth))
    out, stat = _native.dense_attention(q, k, v, heads, precision=CODES[precision], mask=mask_t)
    dq, dk, dv = _native.dense_attention_backward(q, k, v, out, stat, g, heads, precision=CODES[precision], mask=mask_t)
    torch.cuda.synchronize()
    assert tuple(stat.shape) == (N, M, heads, 2)
    return [out, stat[..., 0], stat[..., 1], dq, dk, dv]


def check_parity(config, M, spec, mask_t=None, quantities=range(6)):
    """The kernels against the helper on the mask ``spec``; every figure is printed before it is held to its bound."""
    precision, heads, depth = config
    mask = build_mask(spec, M, heads)
    got = run_native(M, heads, depth, precision, torch.tensor(mask).cuda() if mask_t is None else mask_t)
    want, e_emul = reference(M, heads, depth, spec), emulation_errors(M, heads, depth, spec, precision)
    errs = [rel_err(got[i].cpu().numpy(), want[i]) for i in range(6)]
    print(f"{precision} M {M} {heads}x{depth} {spec}: " + " ".join(f"{NAMES[i]} {errs[i]:.2e}" for i in range(6)))
    for t in got:
        assert bool(torch.isfinite(t).all())
    assert all(np.abs(w).max() > 0 for w in want), "a reference that is zero gives rel_err no scale"
    for i in quantities:
        assert errs[i] <= TOLS[i] + 3 * e_emul[i], f"{NAMES[i]}: {errs[i]:.3e} against {TOLS[i] + 3 * e_emul[i]:.3e}"
    return got


# 1. forward and backward parity, every broadcast form of the mask
@pytest.mark.parametrize("M,form", [(M, form) for M in SIZES for form in FORMS if form != "full" or M <= 65])  # (full: M <= 65)
@pytest.mark.parametrize("config", CONFIGS, ids=config_id)
def test_parity_of_every_mask_form(config, M, form):
    spec = (form, "binary")
    assert_mask_condition(build_mask(spec, M, config[1]), M)
    check_parity(config, M, spec)


# 2. whole tiles masked: the running maximum starts at -1e9 and must rescale to the live tile's
@pytest.mark.parametrize("M,keys", [(331, (0, 64)), (331, (64, 128)), (65, (64, 65))])
@pytest.mark.parametrize("config", CONFIGS, ids=config_id)
def test_whole_tiles_masked(config, M, keys):
    spec = ("key", "keys", keys)
    assert_mask_condition(build_mask(spec, M, config[1]), M)
    check_parity(config, M, spec)


# 3. fully masked rows: uniform softmax, out = mean of v, finite, and gradients that a single lse = m + log l cannot give
@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("config", CONFIGS, ids=config_id)
def test_fully_masked_rows_give_the_mean_of_v(config, M):
    precision, heads, depth = config
    spec = ("pair", "rows")
    mask = build_mask(spec, M, heads)
    assert (mask[0] == 1).all() and (mask[M - 1] == 1).all()
    assert_mask_condition(mask, M, on_purpose=(0, M - 1))
    got = check_parity(config, M, spec)
    v = inputs(M, heads * depth)[2].astype(np.float64)
    mean_v = v.mean(axis=1)  # (N, d): the mean over the keys, per channel (hence per head)
    e_emul = emulation_errors(M, heads, depth, spec, precision)[0]
    for row in (0, M - 1):
        e = rel_err(got[0][:, row].cpu().numpy(), mean_v)
        print(f"  row {row}: out against the mean of v {e:.2e}")
        assert e <= T_OUT + 3 * e_emul
    # the pitfall the pair statistic avoids: in fp32 m + log l is m again on such a row
    m, logl = got[1][:, 0].cpu().numpy(), got[2][:, 0].cpu().numpy()
    assert (m == np.float32(-1e9)).all() and np.allclose(logl, np.log(M), rtol=1e-6, atol=1e-6)
    assert M == 1 or ((m + logl).astype(np.float32) == m).all()


# 4. soft bias: the mask is an add, not a select
@pytest.mark.parametrize("form", ["key", "pair"])
@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("config", CONFIGS, ids=config_id)
def test_soft_bias(config, M, form):
    spec = (form, "soft")
    mask = build_mask(spec, M, config[1])
    bias = mask.astype(np.float32) * np.float32(-1e9)
    assert bias.min() >= -4.001 and bias.max() <= 0 and (M == 2 or bias.min() < -3)  # a select would see "masked" everywhere or nowhere
    check_parity(config, M, spec)


# 5. all-zero mask: the unmasked arithmetic, forward bit for bit
@pytest.mark.parametrize("form", ["key", "pair"])
@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("config", CONFIGS, ids=config_id)
def test_zero_mask_is_the_unmasked_forward_bit_for_bit(config, M, form):
    precision, heads, depth = config
    spec = (form, "zeros")
    got = check_parity(config, M, spec)  # (gradients and statistic: to the tolerances only)
    q, k, v, _ = (torch.as_tensor(a).cuda() for a in inputs(M, heads * depth))
    out, lse = _native.dense_attention(q, k, v, heads, precision=CODES[precision])
    torch.cuda.synchronize()
    assert tuple(lse.shape) == (N, M, heads)  # (the unmasked call keeps its single statistic)
    assert torch.equal(got[0], out)


# 6. reproducibility: two launches, no atomics
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("config", CONFIGS, ids=config_id)
def test_backward_is_bitwise_reproducible(config, form):
    precision, heads, depth = config
    M = 331
    mask_t = torch.tensor(build_mask((form, "binary"), M, heads)).cuda()
    runs = []
    for _ in range(2):
        t = [torch.as_tensor(a).cuda().requires_grad_(True) for a in inputs(M, heads * depth)[:3]]
        out = gnn_transformers.scaled_dot_product_attention(t[0], t[1], t[2], heads, precision=precision, mask=mask_t)
        out.backward(torch.as_tensor(inputs(M, heads * depth)[3]).cuda())
        torch.cuda.synchronize()
        runs.append([out.detach()] + [a.grad for a in t])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# 7. bounds: the mask as a view into a buffer of NaN -- an over-read past a row's end or of a tail key turns the result NaN
def nan_padded(mask, pad, lead):
    """``mask`` (..., M) on the device as a view whose rows are ``pad`` floats longer than M, ``lead`` floats into a NaN buffer."""
    rows = int(np.prod(mask.shape[:-1], dtype=np.int64))
    M = mask.shape[-1]
    buf = torch.full((lead + rows * (M + pad) + 64,), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[lead:lead + rows * (M + pad)].view(rows, M + pad)[:, :M]
    view.copy_(torch.tensor(mask.reshape(rows, M)))
    return view[0] if mask.ndim == 1 else view.unflatten(0, mask.shape[:-1])


@pytest.mark.parametrize("form", ["key", "per_map", "pair"])
@pytest.mark.parametrize("M", [65, 331])
@pytest.mark.parametrize("config", CONFIGS, ids=config_id)
def test_mask_rows_and_tail_keys_are_not_over_read(config, M, form):
    precision, heads, depth = config
    mask = build_mask((form, "binary"), M, heads)
    view = nan_padded(mask, pad=5, lead=3)  # rows 4 (M + 5) bytes apart, the first 12 bytes off the allocation's alignment
    assert view.stride(-1) == 1 and tuple(view.shape) == mask.shape and not bool(torch.isnan(view).any())
    assert form == "key" or not view.is_contiguous()
    t, strides = _native.attention_mask(view, N, heads, M, view.device)
    assert t.data_ptr() == view.data_ptr(), "the view must be read in place for this test to see an over-read"
    got_view = run_native(M, heads, depth, precision, view)
    got = run_native(M, heads, depth, precision, torch.tensor(mask).cuda())
    for name, a, b in zip(NAMES, got_view, got):
        assert bool(torch.isfinite(a).all()), name
        assert torch.equal(a, b), name


# 8. the packed path: MultiHeadAttention(dense=True) with a mask on the strided q | k | v views
def _randomise(layer, seed):
    """Every parameter away from its special initial value (zero biases, unit gains), seeded (as tests/test_gpu_vit.py)."""
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


def compare_with_cpu(label, fn, x, params, g, got_out, got_dx, got_grads):
    """Outputs, input gradient and parameter gradients against ``fn`` in float64, each to ten times the float32 CPU error."""
    out64, dx64, g64 = mref.grads(fn, x, params, g, torch.float64)
    out32, dx32, g32 = mref.grads(fn, x, params, g, torch.float32)
    rows = [("output", got_out, out32, out64)]
    if got_dx is not None:
        rows.append(("dx", got_dx, dx32, dx64))
    rows += [("d " + n, got_grads[n], g32[n], g64[n]) for n in got_grads]
    failed = []
    for name, got, cpu, want in rows:
        e_cpu, e_gpu = rel_err(cpu, want), rel_err(got, want)
        print(f"{label} {name}: cpu-fp32 {e_cpu:.2e} gpu {e_gpu:.2e}")
        assert np.isfinite(got).all()
        if not e_gpu <= 10 * e_cpu:
            failed.append((name, e_gpu, e_cpu))
    assert not failed, f"more than ten times the CPU fp32 error: {failed}"


@pytest.mark.parametrize("form", ["per_map", "pair"])
@pytest.mark.parametrize("precision", ["fp32", "bf16x6"])
def test_multi_head_attention_block_with_a_mask(precision, form):
    M, heads, d = 65, 2, 64
    block = gnn_transformers.MultiHeadAttention(d, heads, dense=True, precision=precision).cuda()
    _randomise(block, 3)
    mask = build_mask((form, "binary"), M, heads)
    rng = np.random.default_rng(21)
    x, g = (rng.standard_normal((N, M, d)).astype(np.float32) for _ in range(2))
    xg = torch.as_tensor(x).cuda().requires_grad_(True)
    out = block(xg, mask=torch.tensor(mask).cuda())
    out.backward(torch.as_tensor(g).cuda())
    torch.cuda.synchronize()
    with torch.no_grad():
        assert not torch.equal(block(xg), out)  # the mask reached the kernel
    params = {n: p.detach().cpu().numpy() for n, p in block.named_parameters()}
    got = {n: p.grad.cpu().numpy() for n, p in block.named_parameters()}
    compare_with_cpu(f"{precision} {form}", lambda xt, p: mref.mha_block(xt, p, "", heads, mask), x, params, g,
                     out.detach().cpu().numpy(), xg.grad.cpu().numpy(), got)


# 9. the layer: Healpy_ViT with a padding mask, at construction, at call time, inside HealpyGCNN
NSIDE, P, KEY_DIM, HEADS, LAYERS, FIN = 8, 1, 16, 2, 2, 3


def footprint_mask(fraction):
    indices = np.arange(healpix.nside2npix(NSIDE))
    footprint = healpix.cap_indices(NSIDE, fraction=fraction)
    mask = healpix.superpixel_padding_mask(indices, footprint, P)
    assert mask.shape == (192,) and 0 < mask.sum() < 192
    return mask


def layer_case(layer, call_mask, used_mask, through=None):
    rng = np.random.default_rng(31)
    x = rng.standard_normal((N, 768, FIN)).astype(np.float32)
    g = rng.standard_normal((N, 192, KEY_DIM * HEADS)).astype(np.float32)
    run = (lambda t: layer(t)) if call_mask is None else (lambda t: layer(t, mask=torch.tensor(call_mask).cuda()))
    if through is not None:
        run = through
    with torch.no_grad():
        run(torch.as_tensor(x).cuda())  # builds the lazily created parameters
    _randomise(layer, 5)
    out = run(torch.as_tensor(x).cuda())
    out.backward(torch.as_tensor(g).cuda())
    torch.cuda.synchronize()
    params = {n: p.detach().cpu().numpy() for n, p in layer.named_parameters()}
    got = {n: p.grad.cpu().numpy() for n, p in layer.named_parameters()}
    assert "mask" not in layer.state_dict()
    compare_with_cpu("Healpy_ViT", lambda xt, p: mref.graph_vit(xt, p, P, HEADS, used_mask, n_layers=LAYERS), x, params, g,
                     out.detach().cpu().numpy(), None, got)
    return out.detach()


def test_healpy_vit_with_a_padding_mask():
    mask = footprint_mask(1.0 / 3.0)
    layer = Healpy_ViT(P, KEY_DIM, HEADS, n_layers=LAYERS, mask=mask)
    masked = layer_case(layer, None, mask)
    assert layer.mask.is_cuda  # (the buffer followed the maps)
    plain = Healpy_ViT(P, KEY_DIM, HEADS, n_layers=LAYERS)
    with torch.no_grad():
        x = torch.as_tensor(np.random.default_rng(31).standard_normal((N, 768, FIN)).astype(np.float32)).cuda()
        plain(x)
        plain.load_state_dict(layer.state_dict())
        assert not torch.equal(plain(x), masked)


def test_the_call_mask_overrides_the_constructor_mask():
    ctor, call = footprint_mask(1.0 / 3.0), footprint_mask(0.6)
    assert not np.array_equal(ctor, call)
    layer_case(Healpy_ViT(P, KEY_DIM, HEADS, n_layers=LAYERS, mask=ctor), call, call)


def test_a_masked_vit_inside_healpy_gcnn():
    mask = footprint_mask(1.0 / 3.0)
    model = deepsphere.HealpyGCNN(NSIDE, np.arange(768), [Healpy_ViT(P, KEY_DIM, HEADS, n_layers=LAYERS, mask=mask)])
    layer_case(model[0], None, mask, through=lambda t: model(t, training=True))
