"""HEALPix-aware layer specs for the Chebyshev path.

Mirror of the reference's ``deepsphere.healpy_layers.HealpyChebyshev``
(``/root/reference/src/deepsphere/healpy_layers.py:219-264``): a deferred description of a
Chebyshev layer that a model builder turns into a real layer once it has computed the graph
Laplacian of the current resolution (``healpy_networks.py:110-137``).
"""

import logging
import os

import numpy as np
import torch

from . import _native, healpix
from .gnn_layers import Bernstein, Chebyshev, GCNN_ResidualLayer, Monomial, _resolve_activation
from .gnn_transformers import Graph_Transformer, Graph_ViT


def _as_tensor(x):
    return x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x), dtype=torch.float32)


class _NestPoolFunction(torch.autograd.Function):
    """HealpyPool on the GPU: ``dsph_healpix_pool`` forward, ``dsph_healpix_pool_backward`` for the input gradient (the
    reference gets the latter from TensorFlow's autodiff of the Keras pooling layer)."""

    @staticmethod
    def forward(ctx, x, group, pool_type):
        ctx.group, ctx.pool_type = group, pool_type
        ctx.save_for_backward(x if pool_type == _native.POOL_MAX else x.new_empty(0))
        return _native.healpix_pool(x, group, pool_type)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return _native.healpix_pool_backward(x if ctx.pool_type == _native.POOL_MAX else None, dy, ctx.group, ctx.pool_type), None, None


class HealpyPool(torch.nn.Module):
    """Pooling over the 4^p NEST children of a HEALPix pixel (reference ``healpy_layers.py:20-78``: a Keras
    MaxPool1D / AveragePooling1D with size = stride = 4^p on (batch, pixels, channels)).  On a HIP device: the
    ``dsph_healpix_pool`` kernels (one contiguous run of 4^p rows per output row); on the CPU (shape checks, tests without a
    GPU) the same reduction as a strided op of the host framework.  It only works for NEST ordering.

    NaN propagates on both branches, for both pooling types: a group with a NaN child pools to NaN (as ``amax`` / ``mean`` on the
    CPU), and the gradient of the maximum goes to the first NaN child.  A layer that reports an out-of-range input as non-finite
    rows (``DSPH_PREC_F16X3``) therefore stays loud behind a ``HealpyPool("MAX")``.  This is a property of this stand-alone layer:
    the convolution + pooling fused in one pass (``dsph_poly_forward_pool``) reduces behind a ReLU that already floors NaN.
    Among equal maxima the gradient goes to the first child in row order."""

    def __init__(self, p, pool_type="MAX", **kwargs):
        super().__init__()
        if not p >= 1:
            raise IOError("The reduction factors has to be at least 2!")
        self.p = p
        self.filter_size = int(4**p)
        self.pool_type = pool_type
        self.kwargs = kwargs
        if pool_type not in ("MAX", "AVG"):
            raise IOError(f"Pooling type not understood: {self.pool_type}")

    def forward(self, input_tensor):
        x = _as_tensor(input_tensor)
        N, M, F = x.shape
        if M % self.filter_size != 0:
            raise IOError(f"Input shape {tuple(x.shape)} not compatible with the filter size {self.filter_size}")
        if x.is_cuda and x.dtype == torch.float32:
            return _NestPoolFunction.apply(x.contiguous(), self.filter_size,
                                           _native.POOL_MAX if self.pool_type == "MAX" else _native.POOL_AVG)
        # (not a HIP float32 tensor -- a CPU tensor, another dtype: the same reduction as a strided op of the host framework.
        # The one host-framework branch of the package, kept for shape checks and tests without a GPU; it is not on the
        # convolution's path and DESIGN.md 1 says so.)
        x = x.reshape(N, M // self.filter_size, self.filter_size, F)
        return x.amax(dim=2) if self.pool_type == "MAX" else x.mean(dim=2)

    call = forward


# arithmetic of the pseudo-convolutions' GEMM by name.  "auto" is the fp32-equivalent six-term split wherever the kernel runs: their
# contractions are short (4^p * Fin down to Fin = 1), where the three-term split measured 1e-5 (gnn_layers.DEFAULT_PRECISION)
_PATCH_PRECISIONS = {"auto": _native.PREC_BF16X6, "fp32": _native.PREC_FP32, "bf16x6": _native.PREC_BF16X6,
                     "bf16x3": _native.PREC_BF16X3}
_PATCH_KWARGS = ("activation", "use_bias", "bias_initializer", "trainable", "name", "precision")
# THE SHAPE RULE of precision="auto": the kernel runs where the contraction is at most 64 long and the output row at most 256
# wide; longer contractions and wider rows keep the library GEMM composition (torch.addmm / @ + bias + activation).  Measured on an
# MI355X against that composition (tools/bench_pseudoconv.py; forward, forward + backward):
#   Kd 4, C 16: 1.38, 1.10    Kd 1, C 64: 1.15, 1.46    Kd 64, C 32: 1.20, 1.64    Kd 16, C 128: 1.64, 1.52    Kd 64, C 256: 1.29, 1.06
#   Kd 256, C 64: 0.80, 0.88  Kd 512, C 32: 0.69, 0.78  Kd 32, C 512: 0.94, 0.93   -- the three that lose, and that the rule excludes
# (at Kd >= 256 the kernel is bound by its split and matrix work, not by the stream).  A precision asked for by name ("fp32",
# "bf16x6", "bf16x3") names the kernel's arithmetic and runs the kernel at every shape in its range.
_PATCH_AUTO_MAX_KD, _PATCH_AUTO_MAX_C = 64, 256


class _PatchGemmFunction(torch.autograd.Function):
    """y = act(x2d @ w2 + bias[c mod P]) on ``dsph_patch_gemm``; the backward is the epilogue's gradient
    (``dsph_patch_epilogue_backward``: dz and dbias), the same GEMM on the transposed weight image for dx and
    ``dsph_cheb_wgrad`` on the one plane x2d for the weight image's gradient.  ``w2`` is the (Kd, C) image of ``filter.weight``; the
    permute that made it carries its gradient back to the parameter's layout."""

    @staticmethod
    def forward(ctx, x2d, w2, bias, P, act, precision, scratch):
        y = _native.patch_gemm(x2d, w2, bias, P, act=act, precision=precision)
        ctx.P, ctx.act, ctx.precision, ctx.has_bias, ctx.scratch = P, act, precision, bias is not None, scratch
        ctx.save_for_backward(x2d, w2, y if act != _native.ACT_NONE else y.new_empty(0))
        return y

    @staticmethod
    def backward(ctx, dy):
        x2d, w2, y = ctx.saved_tensors
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        dz, db = dy.contiguous(), None
        linear = ctx.act == _native.ACT_NONE
        if not linear or need_b:  # (a linear layer without a bias gradient: dz is dy, no launch; with one: dz is dy, a pure reduction)
            dz, db, _ = _native.patch_epilogue_backward(None if linear else y, dz, ctx.P, act=ctx.act, want_dbias=need_b,
                                                        out=dz if linear else None)
        dx = dw = None
        if need_x:
            dx = _native.patch_gemm(dz, w2.t().contiguous(), None, 1, act=_native.ACT_NONE, precision=ctx.precision)
        if need_w:
            R, Kd = x2d.shape
            ws = ctx.scratch.get("wgrad")  # the slabs of dsph_cheb_wgrad, kept on the layer between steps
            dw, ctx.scratch["wgrad"] = _native.cheb_wgrad([x2d.view(1, R, Kd)], dz.view(1, R, dz.shape[1]),
                                                          workspace=ws if ws is not None and ws.device == x2d.device else None)
        return dx, dw, db, None, None, None, None


class _PseudoConvBase(torch.nn.Module):
    """What the two pseudo-convolutions share: the Keras arguments the reference hands to its Conv1D / Conv2DTranspose
    (``activation``, ``use_bias``, ``bias_initializer``, ``trainable``, ``name``), the arithmetic (``precision``: "auto" | "fp32" |
    "bf16x6" | "bf16x3") and the forward: a float32 tensor on a HIP device runs ``dsph_patch_gemm`` with bias and activation in its
    store -- under "auto" (the fp32-equivalent "bf16x6") where the contraction is at most 64 long and the output row at most 256
    wide, the shapes at which it was measured ahead of the library GEMM (``_PATCH_AUTO_MAX_KD``, ``_PATCH_AUTO_MAX_C`` and the
    figures beside them); under a precision asked for by name at every shape the kernel takes.  Anything else (a CPU tensor,
    another dtype, "auto" beyond that rule, a contraction or an output row beyond the kernel's 4096) is the same GEMM as a
    composition of the host framework's operators, bias and activation applied."""

    def _read_kwargs(self, kwargs):
        for key in kwargs:
            if key not in _PATCH_KWARGS:
                raise NotImplementedError(f"{type(self).__name__}: the keyword argument <{key}> is not supported "
                                          f"(supported: {', '.join(_PATCH_KWARGS)})")
        self.activation, self._act_code = _resolve_activation(kwargs.get("activation", None))
        self.use_bias = bool(kwargs.get("use_bias", True))
        self.bias_initializer = kwargs.get("bias_initializer", None)
        self.trainable = bool(kwargs.get("trainable", True))
        self.name = kwargs.get("name", None)
        self.precision = kwargs.get("precision", "auto")
        if self.precision not in _PATCH_PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_PATCH_PRECISIONS)}")
        self._image = None  # inference: (key, the (Kd, C) weight image)
        self._scratch = {}  # training: workspaces kept between steps

    def _init_filter(self):
        torch.nn.init.xavier_uniform_(self.filter.weight)  # Keras default glorot_uniform, zero bias
        if self.filter.bias is not None:
            torch.nn.init.zeros_(self.filter.bias)
        if self.kernel_initializer is not None:
            self.kernel_initializer(self.filter.weight)
        if self.bias_initializer is not None and self.filter.bias is not None:
            self.bias_initializer(self.filter.bias)
        for prm in self.filter.parameters():
            prm.requires_grad_(self.trainable)

    def _weight_image(self, weight):
        raise NotImplementedError

    def _cached_image(self):
        """Inference: the contiguous (Kd, C) image of ``filter.weight``, rebuilt when the parameter was replaced or written in place
        (keyed on ``data_ptr`` and ``_version``, as ``Chebyshev._kernel_image``: a write through ``weight.data``, which bumps no
        version, is not seen -- update the parameter itself under ``torch.no_grad()``)."""
        w = self.filter.weight
        key = (w.data_ptr(), w._version, w.device, w.dtype)
        if self._image is None or self._image[0] != key:
            self._image = (key, self._weight_image(w.detach()).contiguous())
        return self._image[1]

    def _gemm(self, x2d, P):
        """act(x2d @ image + bias by column mod P) for the (R, Kd) view ``x2d`` of the map."""
        weight, bias = self.filter.weight, self.filter.bias
        Kd = int(x2d.shape[1])
        C = weight.numel() // Kd
        native = (x2d.is_cuda and x2d.dtype == torch.float32 and weight.dtype == torch.float32 and weight.device == x2d.device
                  and x2d.shape[0] >= 1 and Kd <= _native.PATCH_MAX_DIM and C <= _native.PATCH_MAX_DIM)
        if native and self.precision == "auto":  # the shape rule (see _PATCH_AUTO_MAX_KD)
            native = Kd <= _PATCH_AUTO_MAX_KD and C <= _PATCH_AUTO_MAX_C
        if not native:
            w2 = self._weight_image(weight).to(x2d.dtype)
            if bias is None:
                y = x2d @ w2
            elif P == C:
                y = torch.addmm(bias.to(x2d.dtype), x2d, w2)
            else:
                y = ((x2d @ w2).reshape(-1, P) + bias.to(x2d.dtype)).reshape(-1, C)
            return y if self.activation is None else self.activation(y)
        act = self._act_code if self._act_code is not None else _native.ACT_NONE
        prec = _PATCH_PRECISIONS[self.precision]
        if torch.is_grad_enabled() and (x2d.requires_grad or weight.requires_grad or (bias is not None and bias.requires_grad)):
            y = _PatchGemmFunction.apply(x2d, self._weight_image(weight).contiguous(), bias, P, act, prec, self._scratch)
        else:
            y = _native.patch_gemm(x2d, self._cached_image(), None if bias is None else bias.detach(), P, act=act, precision=prec)
        return y if self._act_code is not None or self.activation is None else self.activation(y)


class HealpyPseudoConv(_PseudoConvBase):
    """Learnable 4^p -> 1 reduction of NEST children (reference ``healpy_layers.py:81-146``: Conv1D with
    kernel = stride = 4^p, channels last).  Weights: ``filter.weight`` (Fout, Fin, 4^p), ``filter.bias`` (none with
    ``use_bias=False``).  Keyword arguments: see ``_PseudoConvBase``; any other raises ``NotImplementedError``."""

    def __init__(self, p, Fout, kernel_initializer=None, **kwargs):
        super().__init__()
        if not p >= 1:
            raise IOError("The reduction factors has to be at least 1!")
        self.p = p
        self.filter_size = int(4**p)
        self.Fout = Fout
        self.kernel_initializer = kernel_initializer
        self.kwargs = kwargs
        self._read_kwargs(kwargs)
        self.filter = None

    def build(self, input_shape):
        if int(input_shape[1]) % self.filter_size != 0:
            raise IOError(f"Input shape {tuple(input_shape)} not compatible with the filter size {self.filter_size}")
        self.filter = torch.nn.Conv1d(int(input_shape[-1]), self.Fout, self.filter_size, stride=self.filter_size, bias=self.use_bias)
        self._init_filter()

    def _weight_image(self, weight):
        return weight.permute(2, 1, 0).reshape(-1, self.Fout)  # row (i, f) <- weight[o, f, i]

    def forward(self, input_tensor):
        x = _as_tensor(input_tensor)
        if self.filter is None:
            self.build(x.shape)
            self.filter.to(x.device)
        # kernel = stride = 4^p on NEST-ordered rows: the 4^p children of an output pixel are consecutive rows, so the input
        # is, without any copy, a (N * M / 4^p) x (4^p * Fin) matrix and the layer one row GEMM against the
        # [4^p * Fin, Fout] image of the Conv1D weights (no transposes of the map, which Conv1d on channels-last data needs)
        N, M, Fin = x.shape
        g = self.filter_size
        y = self._gemm(x.contiguous().reshape(N * (M // g), g * Fin), self.Fout)
        return y.reshape(N, M // g, self.Fout)

    call = forward


class HealpyPseudoConv_Transpose(_PseudoConvBase):
    """Learnable 1 -> 4^p expansion into NEST children (reference ``healpy_layers.py:149-216``: a
    Conv2DTranspose with kernel = stride = (1, 4^p)).  Weights: ``filter.weight`` (Fin, Fout, 4^p), ``filter.bias`` (none with
    ``use_bias=False``).  Keyword arguments: see ``_PseudoConvBase``; any other raises ``NotImplementedError``."""

    def __init__(self, p, Fout, kernel_initializer=None, **kwargs):
        super().__init__()
        if not p >= 1:
            raise IOError("The boost factors has to be at least 1!")
        self.p = p
        self.filter_size = int(4**p)
        self.Fout = Fout
        self.kernel_initializer = kernel_initializer
        self.kwargs = kwargs
        self._read_kwargs(kwargs)
        self.filter = None

    def build(self, input_shape):
        if int(input_shape[1]) % self.filter_size != 0:  # the reference checks the same thing (:203-204)
            raise IOError(f"Input shape {tuple(input_shape)} not compatible with the filter size {self.filter_size}")
        self.filter = torch.nn.ConvTranspose1d(int(input_shape[-1]), self.Fout, self.filter_size,
                                               stride=self.filter_size, bias=self.use_bias)
        self._init_filter()

    def _weight_image(self, weight):
        return weight.permute(0, 2, 1).reshape(weight.shape[0], -1)  # column (i, o) <- weight[f, o, i]

    def forward(self, input_tensor):
        x = _as_tensor(input_tensor)
        if self.filter is None:
            self.build(x.shape)
            self.filter.to(x.device)
        # the mirror image: every input pixel writes its 4^p NEST children, consecutive rows of the output -- one row GEMM of the
        # (N * M) x Fin map against the [Fin, 4^p * Fout] image of the transposed-convolution weights, the bias periodic in Fout,
        # reshaped for free
        N, M, Fin = x.shape
        y = self._gemm(x.contiguous().reshape(N * M, Fin), self.Fout)
        return y.reshape(N, M * self.filter_size, self.Fout)

    call = forward


class HealpyChebyshev:
    """Deferred spec of a Chebyshev graph convolution on a HEALPix map."""

    def __init__(self, K, Fout=None, initializer=None, activation=None, use_bias=False, use_bn=False, **kwargs):
        """
        :param K: number of polynomial terms
        :param Fout: output channels, defaults to the number of input channels
        :param initializer: weight initialiser, see ``Chebyshev``
        :param activation: activation by name or callable, see ``Chebyshev``
        :param use_bias: learnable bias
        :param use_bn: batch norm before the bias
        :param kwargs: forwarded to the layer
        """
        self.K = K
        self.Fout = Fout  # read by the model builder to track the channel count (healpy_networks.py:160-164)
        self.initializer = initializer
        self.activation = activation
        self.use_bias = use_bias
        self.use_bn = use_bn
        self.kwargs = kwargs

    def _get_layer(self, L, n_matmul_splits=1):
        """Instantiate the layer for graph Laplacian ``L``.

        :param L: the graph Laplacian of the map's pixels (NEST order)
        :param n_matmul_splits: the builder's split count for TensorFlow's sparse matmul; accepted,
            not needed by the HIP kernels
        :return: a callable ``Chebyshev`` layer
        """
        return Chebyshev(
            L=L,
            K=self.K,
            Fout=self.Fout,
            initializer=self.initializer,
            activation=self.activation,
            use_bias=self.use_bias,
            use_bn=self.use_bn,
            n_matmul_splits=n_matmul_splits,
            **self.kwargs,
        )

    _layer_cls = Chebyshev  # the layer this spec instantiates; its ``_scale`` is the one the prepared table must carry

    def _get_layer_prepared(self, cols, vals, lmax, n_matmul_splits=1):
        """The second construction path (``HealpyGCNN(build="device")``): the layer over a Laplacian that is already rescaled
        with ``self._layer_cls._scale`` and laid out as padded ELL (``utils.prepare_ell``), through ``from_prepared_ell`` -- no
        scipy matrix, no eigen-solve.  Such a layer has ``L = None``; ``lmax`` is recorded as given."""
        return self._layer_cls.from_prepared_ell(cols, vals, self.K, lmax=lmax, Fout=self.Fout, initializer=self.initializer,
                                                 activation=self.activation, use_bias=self.use_bias, use_bn=self.use_bn,
                                                 n_matmul_splits=n_matmul_splits, **self.kwargs)


class HealpyMonomial(HealpyChebyshev):
    """Deferred spec of a monomial graph convolution (reference ``healpy_layers.py:267-313``)."""

    _layer_cls = Monomial

    def _get_layer(self, L, n_matmul_splits=1):
        return Monomial(L=L, K=self.K, Fout=self.Fout, initializer=self.initializer, activation=self.activation,
                        use_bias=self.use_bias, use_bn=self.use_bn, n_matmul_splits=n_matmul_splits, **self.kwargs)


class HealpyBernstein(HealpyChebyshev):
    """Deferred spec of a Bernstein graph convolution of order ``K`` (reference ``healpy_layers.py:462``)."""

    _layer_cls = Bernstein

    def _get_layer(self, L, n_matmul_splits=1):
        return Bernstein(L=L, K=self.K, Fout=self.Fout, initializer=self.initializer, activation=self.activation,
                         use_bias=self.use_bias, use_bn=self.use_bn, n_matmul_splits=n_matmul_splits, **self.kwargs)


class Healpy_ResidualLayer:
    """Deferred spec of a residual block of two graph convolutions (reference ``healpy_layers.py:316-378``).

    ``layer_kwargs`` lacks ``L``; ``_get_layer`` adds it (and ``n_matmul_splits``) to a copy -- the reference
    writes them into the caller's dict."""

    def __init__(self, layer_type, layer_kwargs, activation=None, act_before=False, use_bn=False,
                 norm_type="batch_norm", bn_kwargs=None, alpha=1.0):
        self.layer_type = layer_type
        self.layer_kwargs = layer_kwargs
        self.activation = activation
        self.act_before = act_before
        self.use_bn = use_bn
        self.norm_type = norm_type
        self.bn_kwargs = bn_kwargs
        self.alpha = alpha

    def _get_layer(self, L, n_matmul_splits=1):
        kwargs = dict(self.layer_kwargs)
        kwargs.update({"L": L, "n_matmul_splits": n_matmul_splits})
        return GCNN_ResidualLayer(layer_type=self.layer_type, layer_kwargs=kwargs, activation=self.activation,
                                  act_before=self.act_before, use_bn=self.use_bn, norm_type=self.norm_type,
                                  bn_kwargs=self.bn_kwargs, alpha=self.alpha)

    @property
    def _layer_cls(self):
        """The class of the block's two sub-layers (None for a layer type the block does not know: it raises on construction)."""
        return GCNN_ResidualLayer.LAYER_TYPES.get(self.layer_type)

    def _get_layer_prepared(self, cols, vals, lmax, n_matmul_splits=1):
        """As ``HealpyChebyshev._get_layer_prepared``: both sub-layers over the one prepared table (``prepared_ell`` in the
        block's ``layer_kwargs`` in place of ``L``)."""
        kwargs = dict(self.layer_kwargs)
        kwargs.update({"prepared_ell": (cols, vals, lmax), "n_matmul_splits": n_matmul_splits})
        return GCNN_ResidualLayer(layer_type=self.layer_type, layer_kwargs=kwargs, activation=self.activation,
                                  act_before=self.act_before, use_bn=self.use_bn, norm_type=self.norm_type,
                                  bn_kwargs=self.bn_kwargs, alpha=self.alpha)


class Healpy_Transformer:
    """Deferred spec of a graph transformer on a HEALPix map (reference ``healpy_layers.py:417-459``): the model builder hands
    ``_get_layer`` the ADJACENCY matrix of the current resolution, not the Laplacian."""

    def __init__(self, key_dim, num_heads, positional_encoding=True, n_layers=1, activation="relu", layer_norm=True):
        """
        :param key_dim: channels of key, query and value per head; the embedding has ``key_dim * num_heads`` channels
        :param num_heads: number of heads
        :param positional_encoding: add a learned position embedding after the initial embedding
        :param n_layers: number of attention blocks
        :param activation: activation of the blocks
        :param layer_norm: layer norms in the blocks
        """
        self.key_dim = key_dim
        self.num_heads = num_heads
        self.positional_encoding = positional_encoding
        self.n_layers = n_layers
        self.activation = activation
        self.layer_norm = layer_norm
        self.Fout = key_dim * num_heads  # read by the model builder to track the channel count

    def _get_layer(self, A):
        """Instantiate the layer for the graph with adjacency matrix ``A`` (NEST pixel order)."""
        return Graph_Transformer(A=A, key_dim=self.key_dim, num_heads=self.num_heads,
                                 positional_encoding=self.positional_encoding, n_layers=self.n_layers,
                                 activation=self.activation, layer_norm=self.layer_norm)

    def _get_layer_prepared(self, nbr, nbrT):
        """The layer over neighbour tables that exist already (``healpix.healpix_adjacency_tables``); its ``A`` is None."""
        return Graph_Transformer(A=None, key_dim=self.key_dim, num_heads=self.num_heads,
                                 positional_encoding=self.positional_encoding, n_layers=self.n_layers,
                                 activation=self.activation, layer_norm=self.layer_norm, tables=(nbr, nbrT))


class Healpy_ViT(Graph_ViT):
    """``Graph_ViT`` under its HEALPix name (reference ``healpy_layers.py:381-414``, a subclass that adds nothing): a layer, not
    a deferred spec -- it needs no graph.  The model builder counts it as a reduction by 2^p in nside, like ``HealpyPool``."""

    def __init__(self, p, key_dim, num_heads, positional_encoding=True, n_layers=1, activation="relu", layer_norm=True,
                 precision="fp32", mask=None):
        """
        :param p: the super-pixels are the 4^p NEST children of a pixel at nside / 2^p; p >= 1
        :param key_dim: channels of key, query and value per head; the embedding has ``key_dim * num_heads`` channels
        :param num_heads: number of heads
        :param positional_encoding: add a learned position embedding after the initial embedding
        :param n_layers: number of attention blocks
        :param activation: activation of the blocks
        :param layer_norm: layer norms in the blocks
        :param precision: arithmetic of the attention's products: "fp32" (default), "bf16x6" or "bf16x3" -- the bf16 split
            kernels, ``key_dim`` 32 or 64 only (``gnn_transformers.MultiHeadAttention``)
        :param mask: not a reference argument -- the attention mask over the super-pixels used when the call passes none
            (``Graph_ViT``): 1 "do not attend", added to the logits as ``mask * -1e9``; for a footprint padded with
            ``extend_indices``, ``healpix.superpixel_padding_mask(indices, footprint, p)``.  ``forward(inputs, mask=...)``
            overrides it.
        """
        super().__init__(p=p, key_dim=key_dim, num_heads=num_heads, positional_encoding=positional_encoding, n_layers=n_layers,
                         activation=activation, layer_norm=layer_norm, precision=precision, mask=mask)


class _SmoothFunction(torch.autograd.Function):
    """The passes of ``HealpySmoothing`` on the GPU (``dsph_ell_smooth``); the input gradient is the same passes with the
    transposed table, on the upstream gradient times the mask."""

    @staticmethod
    def forward(ctx, x, layer):
        ctx.layer = layer
        cols, vals = layer._tables(x.device)
        return layer._run_passes(x, cols, vals, layer._device_mask(x.device))

    @staticmethod
    def backward(ctx, dy):
        layer = ctx.layer
        mask = layer._device_mask(dy.device)
        g = dy.contiguous() if mask is None else (dy * mask.unsqueeze(0)).contiguous()
        colsT, valsT = layer._transposed_tables(dy.device)
        return layer._run_passes(g, colsT, valsT, None), None


class HealpySmoothing(torch.nn.Module):
    """Smooths a HEALPix map with a Gaussian kernel (reference ``healpy_layers.py:510-853``).

    Every pixel of the patch is replaced by the normalised, Gaussian-weighted sum of its ``max_neighbors`` nearest pixels, where
    ``max_neighbors`` is the largest number of pixels any pixel has within ``n_sigma_support * sigma``.  The smoothing always uses
    one base scale: per-channel scales are reached by applying the kernel ``ceil((s / s_min)^2)`` times (variances add).  The
    kernel matrix is an ELL table of equal-length rows on the GPU (int32 ``cols``, float32 ``vals``, [n_indices, max_neighbors]);
    one pass is one launch of ``dsph_ell_smooth`` over the (batch, pixel, channel) map in place of the reference's per-channel
    sparse matmuls."""

    def __init__(self, nside, indices, nest=True, mask=None, fwhm=None, sigma=None, n_sigma_support=3, arcmin=True,
                 per_channel_repetitions=None, data_path=None, max_batch_size=None, build="host"):
        """
        :param nside: nside of the input maps
        :param indices: 1d array of the NEST pixel ids of the input maps
        :param nest: must be True; RING ordering is not supported
        :param mask: boolean or float array of shape (n_indices,), (n_indices, 1) or (n_indices, n_channels): the output is
            multiplied by it.  None: the maps bleed into the zero padding
        :param fwhm: FWHM of the kernel, a number or one per channel (then the smallest is the base scale)
        :param sigma: the same as a standard deviation; exactly one of ``fwhm`` and ``sigma`` is given.  0 makes the layer the identity
        :param n_sigma_support: radius of the kernel's support in sigmas
        :param arcmin: ``fwhm`` / ``sigma`` are in arcmin (True) or radians
        :param per_channel_repetitions: with a single scale, how often the kernel is applied to each channel
        :param data_path: directory the kernel is loaded from if present and stored to otherwise (``ind_coo<label>.npy``,
            ``val_coo<label>.npy``, the reference's files)
        :param max_batch_size: the reference sizes its sparse-matmul splits by it; the number is computed (``n_matmul_splits``),
            the kernel needs no split
        :param build: not a reference argument -- where the kernel table is built.  "host" (default): a k-d tree over the pixel
            centres, numpy and, for the backward, scipy.  "device": the HIP kernels of ``healpix.gauss_table_device`` on the
            current device (needs a GPU), the transposed table from ``healpix.transpose_table`` on the device; the table never
            visits the host.  Rows hold up to ``_native.DISC_MAX_W`` entries there; beyond, the constructor raises.  At a tied
            ``max_neighbors``-th neighbour the two builds may pick different members of the tie; both tables are correct.  An
            existing ``data_path`` cache is loaded whatever ``build`` says.
        """
        super().__init__()
        if not nest:
            raise NotImplementedError("only NEST ordering is supported")
        if build not in ("host", "device"):
            raise ValueError(f'build = {build!r}: "host" or "device"')
        if build == "device":
            _native.require_gpu()
        self.build_mode = build
        self.completed = 0  # rows of a device build that were completed on the host
        self.nside = nside
        self.indices = indices
        self.nest = nest
        self.mask = mask

        assert fwhm is not None or sigma is not None, "One of fwhm and sigma has to be specified"
        assert fwhm is None or sigma is None, "Only one of fwhm and sigma can be specified"
        self.fwhm = fwhm
        self.sigma = sigma
        self.n_sigma_support = n_sigma_support
        self.arcmin = arcmin
        self.per_channel_repetitions = per_channel_repetitions
        self.data_path = data_path
        self.max_batch_size = max_batch_size
        self.n_channels = None
        self._tables_T = None  # the transposed table: built by the first backward
        self._dev = {}         # per-device copies of reps and mask

        log = logging.getLogger(__name__)
        scalar = lambda v: v is not None and np.ndim(v) == 0
        if (scalar(self.fwhm) and self.fwhm == 0.0) or (scalar(self.sigma) and self.sigma == 0.0):
            self.do_smoothing = False
            log.info("The layer implements the identity, smoothing is disabled")
            return
        self.do_smoothing = True
        if isinstance(self.fwhm, (list, tuple, np.ndarray)):
            assert self.per_channel_repetitions is None, \
                "per_channel_repetitions can't be specified when fwhm is a list, since it is then inferred"
            self.fwhm = np.array(self.fwhm)
            fwhm_min = np.min(self.fwhm)
            # ceil to be conservative, squared because the variances of Gaussians add
            self.per_channel_repetitions = np.ceil((self.fwhm / fwhm_min) ** 2).astype(int)
            self.fwhm = fwhm_min
        elif isinstance(self.sigma, (list, tuple, np.ndarray)):
            assert self.per_channel_repetitions is None, \
                "per_channel_repetitions can't be specified when sigma is a list, since it is then inferred"
            self.sigma = np.array(self.sigma)
            sigma_min = np.min(self.sigma)
            self.per_channel_repetitions = np.ceil((self.sigma / sigma_min) ** 2).astype(int)
            self.sigma = sigma_min
        elif isinstance(self.per_channel_repetitions, (list, tuple)):
            self.per_channel_repetitions = np.array(self.per_channel_repetitions)
        if self.sigma is None:
            self.sigma = self.fwhm / np.sqrt(8 * np.log(2))
        if self.arcmin:
            self.sigma_arcmin = self.sigma
            self.sigma_rad = self._arcmin_to_rad(self.sigma_arcmin)
        else:
            self.sigma_rad = self.sigma
            self.sigma_arcmin = self._rad_to_arcmin(self.sigma_rad)
        self.fwhm_arcmin = self.sigma_arcmin * np.sqrt(8 * np.log(2))
        self.n_indices = len(indices)
        self.kernel_func = lambda r: np.exp(-0.5 / self.sigma_rad**2 * r**2)
        self.file_label = f"-nside{self.nside}-sigma{self.sigma_arcmin:4.2f}-n_sigma{n_sigma_support}"
        if self.per_channel_repetitions is not None:
            log.info(f"Using the per channel smoothing repetitions {self.per_channel_repetitions}")

        ind_coo = val_coo = None
        if self.data_path is not None:
            try:
                ind_coo = np.load(os.path.join(self.data_path, f"ind_coo{self.file_label}.npy"))
                val_coo = np.load(os.path.join(self.data_path, f"val_coo{self.file_label}.npy"))
                log.info(f"Successfully loaded sparse kernel indices and values from {self.data_path}")
            except FileNotFoundError:
                ind_coo = val_coo = None
        if ind_coo is None and build == "device":
            dev = torch.device("cuda", torch.cuda.current_device())
            cols, vals, raw, self.max_neighbors, self.completed = healpix.gauss_table_device(
                self.nside, self.indices, self.sigma_rad, self.n_sigma_support, device=dev, want_raw=self.data_path is not None)
            if self.data_path is not None:
                self._store_kernel(cols.cpu().numpy(), raw.cpu().numpy())
            del raw
            self.register_buffer("cols", cols, persistent=False)
            self.register_buffer("vals", vals, persistent=False)
            return
        if ind_coo is None:
            cols, vals = self._build_tree()
            if self.data_path is not None:
                self._store_kernel(cols, vals)
        else:
            cols, vals = self._table_from_coo(ind_coo, val_coo)
            self.max_neighbors = int(cols.shape[1])
        cols, vals = self._finish_table(cols, vals)
        # non-persistent: the table is derived from the constructor's arguments (and cached by data_path), not learned
        self.register_buffer("cols", torch.from_numpy(cols), persistent=False)
        self.register_buffer("vals", torch.from_numpy(vals), persistent=False)

    # ---- the kernel matrix ---------------------------------------------------------------------------------------------------
    def _build_tree(self):
        """-> (cols int32, vals float32) [n_indices, max_neighbors], every row ordered by distance, values not normalised.
        The reference asks a haversine BallTree; here a k-d tree on the pixels' unit vectors, where a great-circle distance
        theta is the chord 2 sin(theta / 2)."""
        from scipy.spatial import cKDTree

        vec = healpix.pix2vec(self.nside, np.asarray(self.indices, dtype=np.int64))
        tree = cKDTree(vec)
        workers = min(16, os.cpu_count() or 1)
        radius = min(float(self.sigma_rad) * float(self.n_sigma_support), np.pi)
        counts = tree.query_ball_point(vec, 2.0 * np.sin(0.5 * radius), return_length=True, workers=workers)
        self.max_neighbors = int(np.max(counts))
        W, M = self.max_neighbors, self.n_indices
        cols = np.empty((M, W), dtype=np.int32)
        vals = np.empty((M, W), dtype=np.float32)
        step = max(1, (1 << 24) // W)  # rows per query: the float64 distances of a slice stay small
        for a in range(0, M, step):
            chord, ind = tree.query(vec[a:a + step], k=W, workers=workers)
            chord, ind = chord.reshape(-1, W), ind.reshape(-1, W)
            theta = 2.0 * np.arcsin(np.minimum(0.5 * chord, 1.0))
            cols[a:a + step] = ind
            vals[a:a + step] = self.kernel_func(theta).astype(np.float32)
        return cols, vals

    def _store_kernel(self, cols, vals):
        """The reference's files: (nnz, 2) int64 (row, column) pairs and the float32 values before normalisation."""
        M, W = cols.shape
        ind_coo = np.empty((M * W, 2), dtype=np.int64)
        ind_coo[:, 0] = np.repeat(np.arange(M, dtype=np.int64), W)
        ind_coo[:, 1] = cols.reshape(-1)
        os.makedirs(self.data_path, exist_ok=True)
        np.save(os.path.join(self.data_path, f"ind_coo{self.file_label}.npy"), ind_coo)
        np.save(os.path.join(self.data_path, f"val_coo{self.file_label}.npy"), vals.reshape(-1))

    def _table_from_coo(self, ind_coo, val_coo):
        """A stored kernel (entries in any order) as the [n_indices, W] table; every row must hold the same number of entries."""
        M = self.n_indices
        ind_coo, val_coo = np.asarray(ind_coo), np.asarray(val_coo, dtype=np.float32).reshape(-1)
        if ind_coo.ndim != 2 or ind_coo.shape[1] != 2 or ind_coo.shape[0] != val_coo.shape[0]:
            raise ValueError("the stored kernel must be (nnz, 2) indices and (nnz,) values")
        per_row = np.bincount(ind_coo[:, 0], minlength=M)
        W = int(per_row[0]) if M > 0 else 0
        if per_row.shape[0] != M or W < 1 or np.any(per_row != W) or ind_coo[:, 1].min() < 0 or ind_coo[:, 1].max() >= M:
            raise ValueError(f"the stored kernel does not fit a patch of {M} pixels with equally long rows")
        order = np.argsort(ind_coo[:, 0], kind="stable")
        return ind_coo[order, 1].astype(np.int32).reshape(M, W), val_coo[order].reshape(M, W)

    @staticmethod
    def _finish_table(cols, vals):
        """Rows ordered by column (neighbouring lanes of the kernel then read neighbouring pixels) and normalised to sum 1:
        float32 values, their sum taken in float64."""
        M, W = cols.shape
        out_c, out_v = np.empty_like(cols), np.empty_like(vals)
        step = max(1, (1 << 24) // W)
        for a in range(0, M, step):
            c, v = cols[a:a + step], vals[a:a + step]
            order = np.argsort(c, axis=1, kind="stable")
            c, v = np.take_along_axis(c, order, axis=1), np.take_along_axis(v, order, axis=1)
            out_c[a:a + step] = c
            out_v[a:a + step] = (v / v.sum(axis=1, dtype=np.float64, keepdims=True)).astype(np.float32)
        return out_c, out_v

    def _tables(self, device):
        if self.cols.device != device:
            self.cols, self.vals = self.cols.to(device), self.vals.to(device)
        return self.cols, self.vals

    def _transposed_tables(self, device):
        """The table of the transposed matrix, every row padded to the longest with (column = the row itself, value = 0)."""
        if self._tables_T is None and self.build_mode == "device":
            self._tables_T = healpix.transpose_table(*self._tables(device))
        if self._tables_T is None:
            from scipy import sparse

            cols, vals = self.cols.cpu().numpy(), self.vals.cpu().numpy()
            M, W = cols.shape
            K = sparse.csr_matrix((vals.reshape(-1), cols.reshape(-1), np.arange(0, M * W + 1, W)), shape=(M, M))
            K.eliminate_zeros()  # (weights that underflowed: far pixels of the rows at a patch's edge)
            KT = K.T.tocsr()
            KT.sort_indices()
            lens = np.diff(KT.indptr)
            WT = max(int(lens.max()), 1)
            colsT = np.repeat(np.arange(M, dtype=np.int32)[:, None], WT, axis=1)
            valsT = np.zeros((M, WT), dtype=np.float32)
            slot = np.arange(KT.nnz) - np.repeat(KT.indptr[:-1], lens)
            rows = np.repeat(np.arange(M), lens)
            colsT[rows, slot] = KT.indices
            valsT[rows, slot] = KT.data
            self._tables_T = (torch.from_numpy(colsT), torch.from_numpy(valsT))
        if self._tables_T[0].device != device:
            self._tables_T = tuple(t.to(device) for t in self._tables_T)
        return self._tables_T

    # ---- the layer -----------------------------------------------------------------------------------------------------------
    def build(self, input_shape):
        """Checks the input shape (n_batch, n_indices, n_channels) against the layer; brings the mask into shape."""
        if not self.do_smoothing:
            return
        if self.max_batch_size is not None:
            self.n_batch = self.max_batch_size
        elif input_shape[0] is not None:
            self.n_batch = int(input_shape[0])
        else:
            self.n_batch = None
        assert self.n_indices == input_shape[1]
        self.n_channels = int(input_shape[2])
        if self.per_channel_repetitions is not None:
            assert len(self.per_channel_repetitions) == self.n_channels, \
                f"The list per_channel_repetitions has to have length {self.n_channels}"
            assert self.per_channel_repetitions.dtype == int, "The list per_channel_repetitions has to contain integers only"
        if self.mask is not None:
            mask = torch.as_tensor(np.asarray(self.mask.detach().cpu() if isinstance(self.mask, torch.Tensor) else self.mask),
                                   dtype=torch.float32)
            if mask.dim() == 1:
                mask = mask[None, :, None]
            elif mask.dim() == 2:
                mask = mask[None]
            assert mask.dim() == 3 and mask.shape[0] == 1 and mask.shape[1] == self.n_indices and mask.shape[2] in (1, self.n_channels), \
                "The mask has to have shape (1, n_indices, 1) or (1, n_indices, n_channels)"
            self.mask = mask
        # the reference splits its sparse matmul so that no piece passes TensorFlow's int32 limit; one launch here
        self.n_matmul_splits = 1
        if self.n_batch is not None:
            nnz = self.n_indices * self.max_neighbors
            while not (self.n_batch % self.n_matmul_splits == 0 and self.n_matmul_splits >= self.n_batch * nnz / 2**31):
                self.n_matmul_splits += 1
        self._dev = {}

    def _device_mask(self, device):
        """The mask as a contiguous [n_indices, 1 | n_channels] tensor on ``device`` (None without one)."""
        if self.mask is None:
            return None
        key = ("mask", device)
        if key not in self._dev:
            self._dev[key] = self.mask[0].contiguous().to(device)
        return self._dev[key]

    def _device_reps(self, device):
        if self.per_channel_repetitions is None:
            return None
        key = ("reps", device)
        if key not in self._dev:
            self._dev[key] = torch.as_tensor(np.asarray(self.per_channel_repetitions, dtype=np.int32), device=device)
        return self._dev[key]

    def _n_passes(self):
        return 1 if self.per_channel_repetitions is None else int(np.max(self.per_channel_repetitions))

    def _run_passes(self, x, cols, vals, mask):
        """``_n_passes()`` launches, ping-pong between two buffers (a pass cannot run in place); the mask in the last."""
        reps, n = self._device_reps(x.device), self._n_passes()
        bufs = [torch.empty_like(x) for _ in range(min(n, 2))]
        src = x
        for p in range(n):
            src = _native.ell_smooth(cols, vals, src, out=bufs[p % 2], reps=reps, pass_index=p, mask=mask if p == n - 1 else None)
        return src

    def forward(self, inputs):
        """(n_batch, n_indices, n_channels) -> the smoothed maps, same shape."""
        if not self.do_smoothing:
            return inputs
        x = _as_tensor(inputs)
        if self.n_channels is None or x.shape[2] != self.n_channels:
            self.build(tuple(x.shape))
        assert x.dim() == 3 and x.shape[1] == self.n_indices
        if not x.is_cuda:
            raise RuntimeError("HealpySmoothing runs on a HIP device only; there is no CPU fallback")
        x = x.to(torch.float32).contiguous()
        if self._n_passes() == 0:  # every channel passes through
            mask = self._device_mask(x.device)
            return x if mask is None else x * mask.unsqueeze(0)
        return _SmoothFunction.apply(x, self)

    call = forward

    @staticmethod
    def _rad_to_arcmin(theta):
        return theta / np.pi * (180 * 60)

    @staticmethod
    def _arcmin_to_rad(theta):
        return theta * np.pi / (60 * 180)


class _ReorderFunction(torch.autograd.Function):
    """``HealpyReorder``: a permutation of rows; the input gradient is the upstream gradient through the opposite direction of the
    same operator."""

    @staticmethod
    def forward(ctx, x, layer, r2n):
        ctx.layer, ctx.r2n = layer, r2n
        return layer._reorder(x, r2n)

    @staticmethod
    def backward(ctx, dy):
        return ctx.layer._reorder(dy, not ctx.r2n), None, None


# THE SHAPE RULE of HealpyReorder on a full-sky HIP map: the channel counts F for which the table-free kernel
# (dsph_healpix_reorder) is not ahead of dsph_rows_pack on a cached int32 table by more than that contender's own spread run on
# the table instead (tools/bench_reorder.py).  ``_native.healpix_reorder`` always runs the kernel.
def _reorder_on_table(F):
    return False


class HealpyReorder(torch.nn.Module):
    """RING <-> NEST reordering of (batch, pixels, channels) maps as a layer: what the reference's users do with
    ``hp.reorder(m, r2n=True)`` in front of ``HealpyGCNN`` (HEALPix maps are stored in RING order, the network needs NEST) and
    with ``n2r=True`` behind it.  It has no ``p`` and no ``Fout``: ``HealpyGCNN`` passes it through unchanged, so it can stand
    first (``r2n=True``) or last (``r2n=False``) in the list of layers.

    :param nside: nside of the maps
    :param indices: sorted NEST ids of a partial-sky map (the argument of ``HealpyGCNN``), None for the full sky.  The RING side
        of a partial-sky map holds the same pixels sorted by RING id (``indices_ring``)
    :param r2n: True RING -> NEST, False NEST -> RING

    A full-sky float32 map on a HIP device runs the table-free kernel (``dsph_healpix_reorder``; see the shape rule above); a
    partial-sky one ``dsph_rows_pack`` on the int32 table of ``healpix.reorder_table``, moved to the device once; CPU tensors
    (loaders) ``index_select`` on the same table.  Differentiable: the backward is the opposite direction."""

    def __init__(self, nside, indices=None, r2n=True):
        super().__init__()
        self.nside = int(nside)
        if not healpix.isnsideok(self.nside):
            raise ValueError(f"nside = {nside} is not a power of two >= 1")
        self.r2n = bool(r2n)
        self.full_sky = indices is None
        if self.full_sky:
            if self.nside > _native.REORDER_MAX_NSIDE:
                raise ValueError(f"a full-sky map of nside {self.nside} is beyond the int32 pixel indices of the kernel and of the "
                                 f"tables (nside <= {_native.REORDER_MAX_NSIDE}); pass the pixel set as indices")
            self.n_pix = healpix.nside2npix(self.nside)
            self.indices = self.indices_ring = None  # (the whole sky: arange on either side, not materialised)
        else:
            self.indices = np.asarray(indices, dtype=np.int64).reshape(-1)
            self.n_pix = int(self.indices.size)
            self._perm = {}
            self._perm[True], self.indices_ring = healpix.reorder_table(self.nside, self.indices, r2n=True)
            self._perm[False], _ = healpix.reorder_table(self.nside, self.indices, r2n=False)
        self._tables = {}  # (to_nest, device) -> int32 tensor

    def _table(self, to_nest, device):
        key = (bool(to_nest), str(device))
        if key not in self._tables:
            if self.full_sky:
                ids = np.arange(self.n_pix, dtype=np.int64)
                perm = (healpix.nest2ring(self.nside, ids) if to_nest else healpix.ring2nest(self.nside, ids)).astype(np.int32)
            else:
                perm = self._perm[bool(to_nest)]
            self._tables[key] = torch.as_tensor(perm, dtype=torch.int32).to(device)
        return self._tables[key]

    def _reorder(self, x, to_nest):
        if x.is_cuda and x.dtype == torch.float32:
            x = x.contiguous()
            if self.full_sky and not _reorder_on_table(int(x.shape[2])):
                return _native.healpix_reorder(x, self.nside, to_nest)
            return _native.rows_pack(x, self._table(to_nest, x.device))
        return x.index_select(1, self._table(to_nest, x.device))

    def forward(self, input_tensor):
        x = _as_tensor(input_tensor)
        if x.dim() != 3 or x.shape[1] != self.n_pix:
            raise ValueError(f"HealpyReorder: input of shape {tuple(x.shape)} has {x.shape[1] if x.dim() > 1 else 0} pixels, "
                             f"the layer was built for {self.n_pix} (nside {self.nside})")
        return _ReorderFunction.apply(x, self, self.r2n)

    call = forward


class _RotateFunction(torch.autograd.Function):
    """``HealpyRotate``: the interpolation stencil as a gather; the input gradient is the transposed stencil applied to the
    upstream gradient (built in the backward only, so only for an input that requires a gradient)."""

    @staticmethod
    def forward(ctx, x, layer, rot):
        ctx.layer, ctx.rot = layer, rot
        return layer._rotate(x, rot)

    @staticmethod
    def backward(ctx, dy):
        return ctx.layer._rotate_adjoint(dy.contiguous(), ctx.rot), None, None


# THE SHAPE RULE of HealpyRotate with a FIXED rotation on a HIP map: the channel counts F for which the cached W = 4 table through
# dsph_ell_smooth is ahead of the table-free kernel (dsph_healpix_rotate) by more than the kernel's own spread over three
# alternating runs go to the table (tools/bench_rotate.py).  Measured on one MI355X, nside 1024 full sky, one
# rotation for the batch, kernel / ell_smooth on the table built beforehand, ms (the kernel's spread over its three runs):
#   N x F = 8 x 1: 0.606 / 2.038 (0.003);  4 x 4: 0.564 / 1.588 (0.001);  4 x 16: 1.286 / 5.846 (0.003);  2 x 64: 2.502 / 14.263 (0.004)
# The table is ahead in no class, so every F runs the kernel.  (With a workgroup per sample, each computing the same stencils, the
# kernel took 3.353 ms at 8 x 1 and 1.701 at 4 x 4 and the table was ahead in both; the launcher now walks the samples of a shared
# rotation inside the workgroup.)  Rotations drawn per sample always run the kernel -- a table per sample and step is what the
# kernel exists to avoid.
def _rotate_on_table(F):
    return False


class HealpyRotate(torch.nn.Module):
    """Rotates NEST-ordered scalar (batch, pixels, channels) maps by bilinear interpolation on the sphere, what
    ``hp.Rotator.rotate_map_pixel`` does on the host: y(v) = x(R^T v) read through the four-pixel stencil of
    ``healpix.get_interp_weights``.  The augmentation of a training loop on sky maps, on the device.  It has no ``p`` and no
    ``Fout``: ``HealpyGCNN`` passes it through unchanged, so it can stand first in the list of layers.

    :param nside: nside of the maps (at most 8192: pixel ids are int32 in the kernel)
    :param indices: sorted NEST ids of a partial-sky map (the argument of ``HealpyGCNN``), None for the full sky.  A source pixel
        outside the set contributes zero and nothing is renormalised: the rotated zero-padded map, read at the set
    :param rot: "random" -- in ``train()`` mode a fresh rotation, uniform on SO(3), per sample and call
        (``healpix.random_rotations``); in ``eval()`` mode the layer is the identity and returns its input.  Or a [3, 3] rotation
        matrix (``healpix.rotation_matrix``), applied in both modes
    :param generator: the ``torch.Generator`` the random rotations are drawn from (None: the default one of the maps' device)

    ``forward(x, rot=None)``: an explicit [3, 3] or [N, 3, 3] ``rot`` overrides either setting.  Spin-2 fields (shear) do not
    rotate like this; scalar maps only.

    float32 maps on a HIP device run ``dsph_healpix_rotate`` (nothing is materialised; see the shape rule above for a fixed
    rotation); CPU tensors and other dtypes ``healpix.rotation_stencil`` and ``index_select`` on the host.  Differentiable: the input
    gradient is the transposed stencil -- on the device ``_native.healpix_interp_table`` per distinct rotation,
    ``healpix.transpose_table`` and ``_native.ell_smooth`` on the gradient: deterministic, no atomics, and the SLOW path (a table
    per rotation is built after all); an augmentation in front of a network needs no input gradient and never takes it."""

    def __init__(self, nside, indices=None, rot="random", generator=None):
        super().__init__()
        self.nside = int(nside)
        if not healpix.isnsideok(self.nside):
            raise ValueError(f"nside = {nside} is not a power of two >= 1")
        if self.nside > _native.DISC_MAX_NSIDE:
            raise ValueError(f"nside = {self.nside} is beyond the int32 pixel ids of the kernel (nside <= {_native.DISC_MAX_NSIDE})")
        self.indices = healpix._index_set(self.nside, indices)  # None: the full sky
        self.full_sky = self.indices is None
        self.n_pix = healpix.nside2npix(self.nside) if self.full_sky else int(self.indices.size)
        if self.n_pix < 1:
            raise ValueError("an empty pixel set")
        self.generator = generator
        if isinstance(rot, str):
            if rot != "random":
                raise ValueError(f'rot must be "random" or a [3, 3] rotation matrix, got <{rot}>')
            self.rot = None
        else:
            r = np.asarray(rot.detach().cpu() if isinstance(rot, torch.Tensor) else rot, dtype=np.float64)
            if r.shape != (3, 3) or not np.allclose(r.T @ r, np.eye(3), atol=1e-9) or np.linalg.det(r) < 0:
                raise ValueError('rot must be "random" or a [3, 3] rotation matrix (orthonormal, determinant +1)')
            self.rot = torch.as_tensor(r)
        self._sets = {}     # device -> (indices int64, lut int32) of a partial-sky set
        self._fixed = {}    # device -> the fixed rotation there
        self._tables = {}   # (device, transposed) -> the fixed rotation's table there

    def _set(self, device):
        if self.full_sky:
            return None, None
        if str(device) not in self._sets:
            self._sets[str(device)] = healpix._device_lut(self.nside, self.indices, device)
        return self._sets[str(device)]

    def _fixed_table(self, device, transposed):
        key = (str(device), bool(transposed))
        if key not in self._tables:
            table = _native.healpix_interp_table(self.nside, self._fixed[str(device)], *self._set(device), device=device)
            self._tables[key] = healpix.transpose_table(*table) if transposed else table
        return self._tables[key]

    def _host_stencils(self, rot):
        r = rot.detach().cpu().numpy().reshape(-1, 3, 3)
        return [healpix.rotation_stencil(self.nside, ri, self.indices) for ri in r]

    def _rotate(self, x, rot):
        if x.is_cuda and x.dtype == torch.float32:
            x = x.contiguous()
            if rot is self._fixed.get(str(x.device)) and _rotate_on_table(int(x.shape[2])):
                return _native.ell_smooth(*self._fixed_table(x.device, False), x)
            return _native.healpix_rotate(x, self.nside, rot, *self._set(x.device))
        out = torch.zeros_like(x)
        stencils = self._host_stencils(rot)
        for n in range(x.shape[0]):
            rows, w = stencils[n if len(stencils) > 1 else 0]
            for j in range(4):
                rj = torch.as_tensor(rows[j], device=x.device)
                wj = torch.as_tensor(np.where(rows[j] >= 0, w[j], 0.0), device=x.device).to(x.dtype)
                out[n] += x[n].index_select(0, rj.clamp(min=0)) * wj[:, None]
        return out

    def _rotate_adjoint(self, dy, rot):
        if dy.is_cuda and dy.dtype == torch.float32:
            if rot.dim() == 2:
                if rot is self._fixed.get(str(dy.device)):
                    table = self._fixed_table(dy.device, True)
                else:
                    table = healpix.transpose_table(*_native.healpix_interp_table(self.nside, rot, *self._set(dy.device), device=dy.device))
                return _native.ell_smooth(*table, dy)
            dx = torch.empty_like(dy)
            for n in range(dy.shape[0]):
                table = _native.healpix_interp_table(self.nside, rot[n].contiguous(), *self._set(dy.device), device=dy.device)
                _native.ell_smooth(*healpix.transpose_table(*table), dy[n:n + 1], out=dx[n:n + 1])
            return dx
        dx = torch.zeros_like(dy)
        stencils = self._host_stencils(rot)
        for n in range(dy.shape[0]):
            rows, w = stencils[n if len(stencils) > 1 else 0]
            for j in range(4):
                keep = rows[j] >= 0
                rj = torch.as_tensor(rows[j][keep], device=dy.device)
                wj = torch.as_tensor(w[j][keep], device=dy.device).to(dy.dtype)
                dx[n].index_add_(0, rj, dy[n][torch.as_tensor(keep, device=dy.device)] * wj[:, None])
        return dx

    def forward(self, input_tensor, rot=None):
        x = _as_tensor(input_tensor)
        if x.dim() != 3 or x.shape[1] != self.n_pix:
            raise ValueError(f"HealpyRotate: input of shape {tuple(x.shape)} has {x.shape[1] if x.dim() > 1 else 0} pixels, "
                             f"the layer was built for {self.n_pix} (nside {self.nside})")
        N = int(x.shape[0])
        if rot is not None:
            rot = rot if isinstance(rot, torch.Tensor) else torch.as_tensor(np.asarray(rot, dtype=np.float64))
            if tuple(rot.shape) not in ((3, 3), (N, 3, 3)):
                raise ValueError(f"HealpyRotate: rot of shape {tuple(rot.shape)}, expected [3, 3] or [N = {N}, 3, 3]")
            rot = rot.to(device=x.device, dtype=torch.float64).contiguous()
        elif self.rot is not None:
            if str(x.device) not in self._fixed:
                self._fixed[str(x.device)] = self.rot.to(x.device)
            rot = self._fixed[str(x.device)]
        elif not self.training:
            return input_tensor
        else:
            where = x.device if self.generator is None else self.generator.device
            rot = healpix.random_rotations(N, generator=self.generator, device=where).to(x.device)
        return _RotateFunction.apply(x, self, rot)

    call = forward


class HealpyPowerSpectrum(torch.nn.Module):
    """The angular auto power spectrum of NEST-ordered (batch, pixels, channels) maps, what ``hp.anafast`` computes on the host:
    (N, M, F) -> (N, lmax + 1, F), C_l = (|a_l0|^2 + 2 sum_{m > 0} |a_lm|^2) / (2 l + 1) of every map and channel, in the input's
    dtype.  A summary statistic, a loss term or the last layer of a ``HealpyGCNN`` (it has no ``p`` and no ``Fout``: the network
    passes it through unchanged).

    :param nside: nside of the maps (at most 2048)
    :param indices: sorted NEST ids of a partial-sky map, None for the full sky.  On a footprint the result is the pseudo-C_l of
        the zero-filled map: nothing is corrected for the mask
    :param lmax: the largest multipole, 3 nside - 1 by default, at most 4 nside - 1
    :param iter: healpy's Jacobi iterations of ``map2alm`` (0 here by default: the plain quadrature with equal pixel weights)

    float32 maps on a HIP device run the kernels of ``csrc/healpix_sht.hip`` in float64 (``sht.map2alm``); other HIP dtypes are
    converted to float32 first; CPU tensors run the numpy reference without autograd.  Differentiable on the device: at
    ``iter = 0`` the backward is one synthesis, dx = w alm2map(b) with b_lm = 2 gC_l a_lm / (2 l + 1) and w = 4 pi / npix; with
    ``iter > 0`` the composition of the transforms differentiates by itself."""

    def __init__(self, nside, indices=None, lmax=None, iter=0):  # noqa: A002  (healpy's argument name)
        super().__init__()
        self.nside = int(nside)
        if not healpix.isnsideok(self.nside):
            raise ValueError(f"nside = {nside} is not a power of two >= 1")
        if self.nside > _native.SHT_MAX_NSIDE:
            raise ValueError(f"nside = {self.nside} is beyond the transform's limit of {_native.SHT_MAX_NSIDE}")
        self.indices = healpix._index_set(self.nside, indices)  # None: the full sky
        self.n_pix = healpix.nside2npix(self.nside) if self.indices is None else int(self.indices.size)
        if self.n_pix < 1:
            raise ValueError("an empty pixel set")
        self.lmax = healpix._sht_lmax(self.nside, lmax)
        self.iter = int(iter)
        if self.iter < 0:
            raise ValueError(f"iter = {iter} is negative")
        self._footprint = None  # sht.Footprint of the set, with its device tables: built on first use

    def forward(self, input_tensor):
        from . import sht

        x = _as_tensor(input_tensor)
        if x.dim() != 3 or x.shape[1] != self.n_pix:
            raise ValueError(f"HealpyPowerSpectrum: input of shape {tuple(x.shape)} has {x.shape[1] if x.dim() > 1 else 0} pixels, "
                             f"the layer was built for {self.n_pix} (nside {self.nside})")
        if self._footprint is None:
            self._footprint = sht.Footprint(self.nside, self.indices)
        x32 = x.to(torch.float32) if x.is_cuda else x
        return sht.anafast(x32, self.nside, lmax=self.lmax, iter=self.iter, indices=self._footprint).to(x.dtype)

    call = forward


__all__ = ["HealpyPool", "HealpyPseudoConv", "HealpyPseudoConv_Transpose", "HealpyChebyshev", "HealpyMonomial", "HealpyBernstein",
           "Healpy_ResidualLayer", "Healpy_Transformer", "Healpy_ViT", "HealpySmoothing", "HealpyReorder", "HealpyRotate",
           "HealpyPowerSpectrum"]
