"""Graph transformer layers: attention restricted to the edges of the pixel graph, and dense attention over super-pixels.

Mirror of the reference's ``deepsphere.gnn_transformers`` (``gnn_transformers.py``): ``Graph_Transformer`` and ``Graph_ViT`` with
their ``MultiHeadAttention`` blocks and ``AddPositionEmbs``.  The attention over the graph's edges -- in the reference three
embedding lookups that materialise q, k and v per edge, ``exp`` and two segment sums (``:54-106``) -- is one gather kernel forward
and two backward (``csrc/nbr_attention.hip``) working on channels-last (N, M, d) maps and a padded neighbour table.  The dense
attention of ``Graph_ViT`` -- in the reference two ``matmul``s around a softmax over a materialised (N, heads, M, M) tensor
(``:14-51``) -- is a flash-style kernel on the exact-fp32 MFMA (``csrc/dense_attention_kernel.h``, entry points in ``csrc/dense_attention.hip``: key tiles through LDS, online
softmax, no logit in memory; two deterministic backward launches) on the same layout, or, by ``precision=``, on the bf16 MFMA
through a six- or three-term split of its fp32 operands (the same kernels over the arithmetic of ``csrc/dense_attention_split.hip``, depth 32 and 64 per head).  The layer norms around both, with the add
between them, run on the layer-norm kernels (``csrc/layer_norm.hip``); the dense layers are the host framework's, like the GEMM of
``HealpyPseudoConv``.
"""

import numpy as np
import torch
from scipy import sparse

from . import _native
from .gnn_layers import _layer_norm, _resolve_activation
from .utils import adjacency_to_ell


def _as_table(t):
    return t if isinstance(t, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(t, dtype=np.int32))


def neighbour_tables(A):
    """(nbr, nbrT): the neighbour tables (``utils.adjacency_to_ell``) of ``A`` and of ``A.T`` as int32 CPU tensors -- ONE tensor
    when the two are equal, as for every HEALPix graph."""
    A = sparse.csr_matrix(A)
    nbr, nbrT = adjacency_to_ell(A), adjacency_to_ell(A.T)
    nbr = torch.from_numpy(nbr)
    if nbr.shape == nbrT.shape and np.array_equal(nbr.numpy(), nbrT):
        return nbr, nbr
    return nbr, torch.from_numpy(nbrT)


def _tables_from_indices(sparse_A_indices):
    """What ``MultiHeadAttention(sparse_A_indices=...)`` accepts: a pair of neighbour tables (nbr, nbrT), a (sparse) adjacency
    matrix, or the reference's [E, 2] array of (row, column) positions (the graph then has max index + 1 nodes)."""
    if isinstance(sparse_A_indices, (tuple, list)) and len(sparse_A_indices) == 2 and all(
            getattr(t, "ndim", 0) == 2 and "int32" in str(t.dtype) for t in sparse_A_indices):
        return _as_table(sparse_A_indices[0]), _as_table(sparse_A_indices[1])
    if sparse.issparse(sparse_A_indices):
        return neighbour_tables(sparse_A_indices)
    idx = np.asarray(sparse_A_indices)
    if idx.ndim == 2 and idx.shape[1] == 2 and np.issubdtype(idx.dtype, np.integer):
        M = int(idx.max()) + 1 if idx.size else 0
        return neighbour_tables(sparse.csr_matrix((np.ones(idx.shape[0]), (idx[:, 0], idx[:, 1])), shape=(M, M)))
    if idx.ndim == 2 and idx.shape[0] == idx.shape[1]:
        return neighbour_tables(sparse.csr_matrix(idx))
    raise ValueError("sparse_A_indices: expected (nbr, nbrT) int32 tables, an adjacency matrix or an [E, 2] index array")


def _kernel_layout(q, k, v):
    """q, k, v as the kernel reads them: untouched when they are rows of one common stride (contiguous, or channel slices of one
    projection buffer), contiguous copies otherwise."""
    lds = [_native.rows_layout(t) for t in (q, k, v)]
    ok = None not in lds and len(set(lds)) == 1 and lds[0] % 4 == 0 and all(t.data_ptr() % 16 == 0 for t in (q, k, v))
    return (q, k, v) if ok else (q.contiguous(), k.contiguous(), v.contiguous())


def _require_hip(*tensors):
    _native.require_gpu()
    for t in tensors:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3):
            raise ValueError("the neighbour attention works on float32 HIP tensors (N, M, d); there is no CPU path")


class _SparseAttention(torch.autograd.Function):
    """out = softmax over the neighbours of (q k^T / sqrt(depth)) v; saves q, k, v, out and the log-sum-exp, gradients from
    ``dsph_nbr_attention_backward``."""

    @staticmethod
    def forward(ctx, q, k, v, nbr, nbrT, num_heads):
        q, k, v = _kernel_layout(q, k, v)
        out, lse = _native.nbr_attention(q, k, v, nbr, num_heads)
        ctx.save_for_backward(q, k, v, out, lse, nbr, nbrT)
        ctx.num_heads = num_heads
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse, nbr, nbrT = ctx.saved_tensors
        dq, dk, dv = _native.nbr_attention_backward(q, k, v, out, lse, dout, nbr, nbrT, ctx.num_heads)
        return dq, dk, dv, None, None, None


class _SparseAttentionPacked(torch.autograd.Function):
    """The same on the output of a fused projection, qkv (N, M, 3 d) = [q | k | v]: the kernels read the three channel slices in
    place and write dq, dk, dv into the slices of ONE gradient tensor (autograd would otherwise pad and add three of them)."""

    @staticmethod
    def forward(ctx, qkv, nbr, nbrT, num_heads):
        qkv = qkv.contiguous()
        d = qkv.shape[2] // 3
        q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
        if d % 4 != 0:  # (slices that are not 16-byte aligned: copies; the kernels then name their limit)
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        out, lse = _native.nbr_attention(q, k, v, nbr, num_heads)
        ctx.save_for_backward(qkv, out, lse, nbr, nbrT)
        ctx.num_heads = num_heads
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse, nbr, nbrT = ctx.saved_tensors
        d = qkv.shape[2] // 3
        dqkv = torch.empty_like(qkv)
        _native.nbr_attention_backward(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], out, lse, dout, nbr, nbrT, ctx.num_heads,
                                       grads=(dqkv[..., :d], dqkv[..., d:2 * d], dqkv[..., 2 * d:]))
        return dqkv, None, None, None


# The arithmetic of the dense-attention products, by name.  "fp32": the exact-fp32 MFMA, every depth.  "bf16x6" (fp32-equivalent)
# and "bf16x3": the bf16 split kernels, depth 32 and 64 per head only.  There is no "auto" and nothing falls back.
_DENSE_PRECISIONS = {"fp32": _native.PREC_FP32, "bf16x6": _native.PREC_BF16X6, "bf16x3": _native.PREC_BF16X3}
_SPLIT_DEPTHS = (32, 64)


def _dense_precision(precision, depth=None):
    """The name of a dense-attention arithmetic, checked (and, with ``depth``, checked against the depths it runs)."""
    if precision not in _DENSE_PRECISIONS:
        raise ValueError(f"precision = {precision!r} is not one of 'fp32', 'bf16x6', 'bf16x3'")
    if precision != "fp32" and depth is not None and depth not in _SPLIT_DEPTHS:
        raise ValueError(f"precision = {precision!r} runs key_dim (channels per head) 32 or 64, not {depth}: the bf16 split "
                         "kernels contract 32 channels per instruction; use precision='fp32'")
    return precision


def _dense_mask(mask, N, num_heads, M, device):
    """The mask of a dense-attention call as the kernels read it (``_native.attention_mask``), or None."""
    return None if mask is None else _native.attention_mask(mask, N, num_heads, M, device)[0]


class _DenseAttention(torch.autograd.Function):
    """out = softmax over ALL rows of (q k^T / sqrt(depth) + mask * -1e9) v; saves q, k, v, out and the log-sum-exp -- with a mask
    the mask and the statistic pair (m, log l) -- gradients from ``dsph_dense_attention_backward`` / ``_backward_masked``.  The
    mask gets no gradient."""

    @staticmethod
    def forward(ctx, q, k, v, num_heads, precision=_native.PREC_FP32, mask=None):
        q, k, v = _kernel_layout(q, k, v)
        mask = _dense_mask(mask, q.shape[0], num_heads, q.shape[1], q.device)
        out, lse = _native.dense_attention(q, k, v, num_heads, precision=precision, mask=mask)
        ctx.save_for_backward(q, k, v, out, lse, mask)
        ctx.num_heads, ctx.precision = num_heads, precision
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse, mask = ctx.saved_tensors
        dq, dk, dv = _native.dense_attention_backward(q, k, v, out, lse, dout, ctx.num_heads, precision=ctx.precision, mask=mask)
        return dq, dk, dv, None, None, None


class _DenseAttentionPacked(torch.autograd.Function):
    """The same on the output of a fused projection, qkv (N, M, 3 d) = [q | k | v], like ``_SparseAttentionPacked``: three channel
    slices read in place, dq, dk, dv written into the slices of ONE gradient tensor."""

    @staticmethod
    def forward(ctx, qkv, num_heads, precision=_native.PREC_FP32, mask=None):
        qkv = qkv.contiguous()
        d = qkv.shape[2] // 3
        q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
        if d % 4 != 0:  # (slices that are not 16-byte aligned: copies; the kernels then name their limit)
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        mask = _dense_mask(mask, qkv.shape[0], num_heads, qkv.shape[1], qkv.device)
        out, lse = _native.dense_attention(q, k, v, num_heads, precision=precision, mask=mask)
        ctx.save_for_backward(qkv, out, lse, mask)
        ctx.num_heads, ctx.precision = num_heads, precision
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse, mask = ctx.saved_tensors
        d = qkv.shape[2] // 3
        dqkv = torch.empty_like(qkv)
        _native.dense_attention_backward(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], out, lse, dout, ctx.num_heads,
                                         grads=(dqkv[..., :d], dqkv[..., d:2 * d], dqkv[..., 2 * d:]), precision=ctx.precision,
                                         mask=mask)
        return dqkv, None, None, None


def scaled_dot_product_attention(q, k, v, num_heads, precision="fp32", mask=None):
    """Attention of every row over all rows of its map (reference ``gnn_transformers.py:14-51``), differentiable in q, k, v.

    :param q, k, v: float32 HIP tensors (N, M, d), channels last; head h is channels [h d / num_heads, (h + 1) d / num_heads)
        -- the reference's ``split_heads`` without its transposes.  Strided views are read in place when their rows share one
        stride (three slices of one projection buffer).
    :param num_heads: number of heads; d / num_heads one of 4, 8, 16, 32, 64 and d <= 256
    :param precision: not a reference argument -- the arithmetic of the products: "fp32" (exact-fp32 MFMA), "bf16x6" (bf16 MFMA
        on a three-term split of both operands, fp32-equivalent) or "bf16x3" (two terms, operands to 16 bits); the split ones
        run d / num_heads 32 and 64 only and raise elsewhere
    :param mask: the reference's argument: a float tensor that broadcasts against the (N, heads, M, M) logits and is added to them
        as ``mask * -1e9`` before the softmax, inside the kernel, in all three arithmetics on the fp32 logit -- 1 "do not attend",
        0 "attend", a fraction a soft bias (an add, not a select).  Any broadcast form: a key mask (M,), per map (N, 1, 1, M), per
        head (1, heads, 1, M), a pair mask (M, M), a full one; the kernels broadcast by stride, nothing of size N heads M M is
        allocated for a broadcast mask, and views are read in place.  bool / int masks are converted to float32.  Not
        differentiable: a mask that requires grad raises, as does a shape that does not broadcast.  A row whose keys are all
        masked gives the mean of v, as in the reference (-1e9 absorbs any logit below 32 in fp32).  None (default): the unmasked
        kernels, unchanged.
    :return: (N, M, d)

    The reference also returns the attention weights, an (N, heads, M, M) tensor that nothing in it reads; they are never formed
    here (that is the point of the kernel)."""
    if mask is not None and isinstance(mask, torch.Tensor) and mask.requires_grad:
        raise ValueError("the attention mask is not differentiable (it enters the logits as mask * -1e9): pass mask.detach()")
    _require_hip(q, k, v)
    code = _DENSE_PRECISIONS[_dense_precision(precision)]
    if mask is None:
        return _DenseAttention.apply(q, k, v, int(num_heads), code)
    return _DenseAttention.apply(q, k, v, int(num_heads), code, _dense_mask(mask, q.shape[0], int(num_heads), q.shape[1], q.device))


def scaled_dot_product_sparse_attention(q, k, v, nbr, nbrT, num_heads):
    """Attention of every pixel over its graph neighbours (reference ``gnn_transformers.py:54-106``), differentiable.

    :param q, k, v: float32 HIP tensors (N, M, d), channels last; head h is channels [h d / num_heads, (h + 1) d / num_heads)
        -- the reference's ``split_heads`` without its transposes.  Strided views are read in place when their rows share one
        stride (three slices of one projection buffer).
    :param nbr: int32 [M, W] neighbour table (``utils.adjacency_to_ell(A)``), on the tensors' device
    :param nbrT: the table of ``A.T`` (the same tensor for a symmetric graph); read by the backward only
    :param num_heads: number of heads
    :return: (N, M, d)

    The softmax is evaluated in its stable form (running maximum), a deliberate deviation from the reference, which
    exponentiates the raw logits and overflows in fp32 once one exceeds about 88; mathematically the two are equal.  A row
    without neighbours gives zeros (the reference: 0 / 0)."""
    _require_hip(q, k, v)
    return _SparseAttention.apply(q, k, v, nbr, nbrT, int(num_heads))


def _glorot_uniform_(w):
    torch.nn.init.xavier_uniform_(w)  # Keras' default glorot_uniform: limit = sqrt(6 / (fan_in + fan_out))


class AddPositionEmbs(torch.nn.Module):
    """Adds a learned positional embedding (1, M, d) to the input (reference ``gnn_transformers.py:113-146``); built on the
    first call.  Default initialiser: Glorot-uniform with Keras' fans for that shape, limit = sqrt(6 / (M + d)) (the reference
    passes ``posemb_init=None``, Keras' default for ``add_weight``)."""

    def __init__(self, posemb_init=None, **kwargs):
        super().__init__()
        self.posemb_init = posemb_init
        self.pos_embedding = None

    def build(self, inputs_shape, device=None):
        M, d = int(inputs_shape[1]), int(inputs_shape[2])
        w = torch.empty((1, M, d), dtype=torch.float32, device=device)
        if self.posemb_init is not None:
            self.posemb_init(w)
        else:
            limit = float(np.sqrt(6.0 / (M + d)))
            torch.nn.init.uniform_(w, -limit, limit)
        self.pos_embedding = torch.nn.Parameter(w)

    def forward(self, inputs):
        if self.pos_embedding is None:
            self.build(inputs.shape, inputs.device)
        return inputs + self.pos_embedding.to(inputs.dtype)

    call = forward


class MultiHeadAttention(torch.nn.Module):
    """One transformer block of the reference (``gnn_transformers.py:149-245``), in its order: layer norm, q / k / v projections,
    attention over the graph neighbours, + the normed input, layer norm, dense, activation, + the residual again.

    Parameters: ``wqkv`` -- the reference's three ``Dense(d_model)`` layers ``wq``, ``wk``, ``wv`` fused into ONE [d, 3 d]
    projection (rows [0, d) of ``wqkv.weight`` are wq, [d, 2 d) wk, [2 d, 3 d) wv; each block Glorot-uniform with its own
    fans, zero bias), whose output the kernel reads as three strided views -- ``dense``, ``layer_norm1``, ``layer_norm2``
    (eps = 1e-3, Keras' default).  ``use_norm=False`` makes both norms the identity (the reference crashes there: it calls
    norms it did not create)."""

    def __init__(self, d_model, num_heads, use_norm=True, activation="relu", sparse_A_indices=None, dense=False, precision="fp32"):
        """
        :param d_model: channels of q, k and v (all heads together)
        :param num_heads: number of heads; must divide ``d_model``
        :param use_norm: layer norms, or identities
        :param activation: by Keras name or a callable
        :param sparse_A_indices: the graph -- a pair of neighbour tables (nbr, nbrT), an adjacency matrix or the reference's
            [E, 2] positions.  None: the tables must come with the call (``Graph_Transformer`` passes its own), or ``dense``
            must be set.
        :param dense: not a reference argument -- attention over ALL rows on the dense kernel (what the reference does when it has
            no ``sparse_A_indices``; ``Graph_ViT`` builds its blocks this way).  No tables are needed or read.  The reference's
            ``mask`` argument of that path comes with the call (``forward``).
        :param precision: not a reference argument -- the arithmetic of the dense attention's products, "fp32" (default),
            "bf16x6" or "bf16x3" (``scaled_dot_product_attention``).  A split one needs ``dense=True`` and 32 or 64 channels per
            head; the attention over graph neighbours is a memory-bound gather and has no split.
        """
        super().__init__()
        if num_heads < 1 or d_model % num_heads != 0:
            raise ValueError(f"d_model = {d_model} must be a multiple of num_heads = {num_heads}")
        self.d_model, self.num_heads, self.use_norm = int(d_model), int(num_heads), bool(use_norm)
        self.depth = self.d_model // self.num_heads
        self.dense_attention = bool(dense)
        self.precision = _dense_precision(precision, self.depth)
        if self.precision != "fp32" and not self.dense_attention:
            raise ValueError(f"precision = {precision!r} needs dense=True: the attention over graph neighbours has no split "
                             "arithmetic")
        self.activation, self._act_code = _resolve_activation(activation)
        if sparse_A_indices is not None:
            nbr, nbrT = _tables_from_indices(sparse_A_indices)
            self.register_buffer("nbr", nbr, persistent=False)
            if nbrT is not nbr:
                self.register_buffer("nbrT_", nbrT, persistent=False)
        else:
            self.nbr = None
        d = self.d_model
        self.wqkv = torch.nn.Linear(d, 3 * d)
        self.dense = torch.nn.Linear(d, d)
        with torch.no_grad():
            for i in range(3):
                _glorot_uniform_(self.wqkv.weight[i * d:(i + 1) * d])
            _glorot_uniform_(self.dense.weight)
            self.wqkv.bias.zero_()
            self.dense.bias.zero_()
        if self.use_norm:
            self.layer_norm1 = torch.nn.LayerNorm(d, eps=1e-3)
            self.layer_norm2 = torch.nn.LayerNorm(d, eps=1e-3)
        else:
            self.layer_norm1 = torch.nn.Identity()
            self.layer_norm2 = torch.nn.Identity()

    @property
    def nbrT(self):
        return getattr(self, "nbrT_", self.nbr)

    def forward(self, inputs, tables=None, mask=None):
        """``mask``: the reference's ``call(inputs, mask=None)`` argument, for the dense path (``dense=True``): see
        ``scaled_dot_product_attention``.  Deviation from the reference: on the path over graph neighbours the reference accepts a
        mask and silently ignores it; here that raises ValueError -- a mask that is dropped is a data bug, and there the
        neighbour table is the mask."""
        nbr, nbrT = (None, None) if self.dense_attention else tables if tables is not None else (self.nbr, self.nbrT)
        if nbr is None and not self.dense_attention:
            raise NotImplementedError("MultiHeadAttention without neighbour tables is dense attention over all pixels (the "
                                      "reference's Graph_ViT path): construct the block with dense=True to run it")
        if mask is not None and not self.dense_attention:
            raise ValueError("mask: the attention over graph neighbours takes no mask (the neighbour table is the mask; the "
                             "reference ignores the argument there): construct the block with dense=True")
        if mask is not None and isinstance(mask, torch.Tensor) and mask.requires_grad:
            raise ValueError("the attention mask is not differentiable (it enters the logits as mask * -1e9): pass mask.detach()")
        _require_hip(inputs)
        # the norms run on the layer-norm kernels (csrc/layer_norm.hip), the add between them inside the second one's launch
        x = _layer_norm(self.layer_norm1, inputs) if self.use_norm else inputs
        qkv = self.wqkv(x)  # (N, M, 3 d): q | k | v
        if self.dense_attention:
            if mask is None:
                att = _DenseAttentionPacked.apply(qkv, self.num_heads, _DENSE_PRECISIONS[self.precision])
            else:
                att = _DenseAttentionPacked.apply(qkv, self.num_heads, _DENSE_PRECISIONS[self.precision], mask)
        else:
            att = _SparseAttentionPacked.apply(qkv, nbr, nbrT, self.num_heads)
        if self.use_norm:
            y, att = _layer_norm(self.layer_norm2, att, x)  # att <- x + att, y = LN(att): one pass
        else:
            att = x + att
            y = att
        out = self.dense(y)
        # without autograd the tail act(out) + att is ONE pass in place over the GEMM's fresh output (dsph_residual_epilogue);
        # with autograd on, or an activation the kernels have no code for, the host framework composes it
        if (not (torch.is_grad_enabled() and (out.requires_grad or att.requires_grad)) and out.dtype == torch.float32
                and (self.activation is None or self._act_code is not None) and out.is_contiguous()):
            return _native.residual_epilogue(out, att.contiguous(), 1.0, _native.ACT_NONE if self.activation is None else self._act_code, True)
        if self.activation is not None:
            out = self.activation(out)
        return out + att

    call = forward


class Graph_Transformer(torch.nn.Module):
    """A graph transformer on the pixels of a map (reference ``gnn_transformers.py:359-450``): a dense embedding to
    ``key_dim * num_heads`` channels, an optional learned position embedding and ``n_layers`` attention blocks whose softmax
    runs over the edges of the adjacency matrix ``A`` (only its pattern is used).

    Parameter names follow the reference's attributes: ``embed``, ``pos_encoder.pos_embedding``,
    ``mha_layers.{i}.wqkv / dense / layer_norm1 / layer_norm2`` (``wqkv``: wq, wk, wv fused, see ``MultiHeadAttention``).
    ``embed`` and the position embedding are built on the first call, like Keras builds them.  Runs on a HIP device only."""

    def __init__(self, A, key_dim, num_heads, positional_encoding=True, n_layers=1, activation="relu", layer_norm=True, tables=None):
        """``tables`` (not a reference argument): the int32 neighbour tables (nbr, nbrT) of the graph where they exist already
        (``healpix.healpix_adjacency_tables``; the same tensor twice for a symmetric graph); ``A`` is then not read and may be None."""
        super().__init__()
        if not n_layers >= 1:
            raise ValueError("Number of attention layers should be at least 1")
        self.A = A
        self.key_dim, self.num_heads = int(key_dim), int(num_heads)
        self.embedding_size = self.key_dim * self.num_heads
        self.Fout = self.embedding_size  # read by the model builder to track the channel count
        self.positional_encoding = positional_encoding
        self.n_layers = n_layers
        self.activation = activation
        self.layer_norm = layer_norm
        if tables is None:
            nbr, nbrT = neighbour_tables(A)
        else:
            nbr, nbrT = tables
            for t in (nbr, nbrT):
                if not (isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.dim() == 2 and t.is_contiguous()):
                    raise ValueError("tables: expected (nbr, nbrT) contiguous int32 tensors [M, W]")
        self.register_buffer("nbr", nbr, persistent=False)
        if nbrT is not nbr:
            self.register_buffer("nbrT_", nbrT, persistent=False)
        self.embed = None
        if self.positional_encoding:
            self.pos_encoder = AddPositionEmbs()
        self.mha_layers = torch.nn.ModuleList(
            MultiHeadAttention(d_model=self.embedding_size, num_heads=self.num_heads, use_norm=self.layer_norm,
                               activation=self.activation) for _ in range(n_layers))

    @property
    def nbrT(self):
        return getattr(self, "nbrT_", self.nbr)

    def build(self, input_shape, device=None):
        self.embed = torch.nn.Linear(int(input_shape[-1]), self.embedding_size, device=device)
        with torch.no_grad():
            _glorot_uniform_(self.embed.weight)
            self.embed.bias.zero_()
        if self.positional_encoding and self.pos_encoder.pos_embedding is None:
            self.pos_encoder.build((1, int(input_shape[1]), self.embedding_size), device)

    def forward(self, inputs):
        x = inputs if isinstance(inputs, torch.Tensor) else torch.as_tensor(np.asarray(inputs), dtype=torch.float32)
        _require_hip(x)
        if x.shape[1] != self.nbr.shape[0]:
            raise ValueError(f"the input has {x.shape[1]} pixels, the graph {self.nbr.shape[0]}")
        if self.embed is None:
            self.build(x.shape, x.device)
        if self.nbr.device != x.device:  # (the tables follow the maps, like the plans of the convolution layers)
            self.nbr = self.nbr.to(x.device)
            if hasattr(self, "nbrT_"):
                self.nbrT_ = self.nbrT_.to(x.device)
        for m in self.mha_layers:  # (lazily built layers: parameters created before a .to(device) of the parent are moved by it)
            if m.wqkv.weight.device != x.device:
                m.to(x.device)
        x = self.embed(x)
        if self.positional_encoding:
            x = self.pos_encoder(x)
        tables = (self.nbr, self.nbrT)
        for mha in self.mha_layers:
            x = mha(x, tables)
        return x

    call = forward


class Graph_ViT(torch.nn.Module):
    """A vision transformer on the super-pixels of a map (reference ``gnn_transformers.py:248-356``): the 4^p NEST children of
    a pixel of the p-times coarser map are one patch, embedded to ``key_dim * num_heads`` channels by a Conv1D with
    kernel = stride = 4^p, an optional learned position embedding, then ``n_layers`` attention blocks in which every super-pixel
    attends to every other one (``MultiHeadAttention(dense=True)``, the flash-style kernel).  The layer reduces the pixel count
    by 4^p; it only checks that the count is a multiple of 4^p, not the ordering (NEST).

    ``p >= 1`` is accepted: the reference's check ``not p > 1`` rejects p = 1 and so contradicts its own message ("has to be at
    least 1") and its docstring; p = 1 is a valid patch of four pixels.

    Parameter names follow the reference's attributes: ``embed.weight`` (d, Fin, 4^p) and ``embed.bias`` -- a lazily built
    ``torch.nn.Conv1d``, Glorot-uniform / zero like Keras, evaluated as a single ``addmm`` on the free reshape ``HealpyPseudoConv`` makes --
    ``pos_encoder.pos_embedding`` (1, M / 4^p, d) and ``mha_layers.{i}.wqkv / dense / layer_norm1 / layer_norm2`` as in
    ``Graph_Transformer``.  Runs on a HIP device only.

    ``mask``: the reference's blocks take ``call(inputs, mask=None)`` but its ``Graph_ViT`` never passes one; here
    ``forward(inputs, mask=None)`` hands the mask (over the SUPER-pixels: it broadcasts against (N, heads, M / 4^p, M / 4^p), see
    ``scaled_dot_product_attention``) to every block.  The constructor argument ``mask`` is not a reference argument: it is kept
    as a non-persistent buffer (it follows ``.to(device)``, stays out of the ``state_dict``) and used whenever the call passes
    none, so that a masked layer can sit inside ``HealpyGCNN``, whose ``forward`` hands its layers the maps alone.  For a padded
    survey footprint ``healpix.superpixel_padding_mask`` builds the key mask."""

    def __init__(self, p, key_dim, num_heads, positional_encoding=True, n_layers=1, activation="relu", layer_norm=True,
                 precision="fp32", mask=None):
        super().__init__()
        if not p >= 1:
            raise IOError("The super pixel size factor p has to be at least 1!")
        if not n_layers >= 1:
            raise ValueError("Number of attention layers should be at least 1")
        self.p = p
        self.embed_filter_size = int(4 ** p)
        self.key_dim, self.num_heads = int(key_dim), int(num_heads)
        self.embedding_size = self.key_dim * self.num_heads
        self.Fout = self.embedding_size  # read by the model builder to track the channel count
        self.positional_encoding = positional_encoding
        self.n_layers = n_layers
        self.activation = activation
        self.layer_norm = layer_norm
        self.precision = _dense_precision(precision, int(key_dim))  # (of the blocks' attention; see MultiHeadAttention)
        if mask is not None:
            mask = mask if isinstance(mask, torch.Tensor) else torch.as_tensor(np.asarray(mask))
            if mask.requires_grad:
                raise ValueError("the attention mask is not differentiable (it enters the logits as mask * -1e9): pass mask.detach()")
            if mask.dim() < 1 or mask.dim() > 4:
                raise ValueError(f"mask of shape {tuple(mask.shape)} does not broadcast against the logits (N, heads, M, M)")
            mask = mask.detach().to(torch.float32)
        self.register_buffer("mask", mask, persistent=False)
        self.embed = None
        if self.positional_encoding:
            self.pos_encoder = AddPositionEmbs()
        self.mha_layers = torch.nn.ModuleList(
            MultiHeadAttention(d_model=self.embedding_size, num_heads=self.num_heads, use_norm=self.layer_norm,
                               activation=self.activation, dense=True, precision=self.precision) for _ in range(n_layers))

    def build(self, input_shape, device=None):
        n_nodes, g = int(input_shape[1]), self.embed_filter_size
        if n_nodes % g != 0:
            raise IOError(f"Input shape {tuple(input_shape)} not compatible with the embedding filter size {g}")
        self.embed = torch.nn.Conv1d(int(input_shape[-1]), self.embedding_size, g, stride=g, device=device)
        with torch.no_grad():
            _glorot_uniform_(self.embed.weight)
            self.embed.bias.zero_()
        if self.positional_encoding and self.pos_encoder.pos_embedding is None:
            self.pos_encoder.build((1, n_nodes // g, self.embedding_size), device)

    def forward(self, inputs, mask=None):
        x = inputs if isinstance(inputs, torch.Tensor) else torch.as_tensor(np.asarray(inputs), dtype=torch.float32)
        g = self.embed_filter_size
        if x.dim() == 3 and x.shape[1] % g != 0:
            raise IOError(f"Input shape {tuple(x.shape)} not compatible with the embedding filter size {g}")
        _require_hip(x)
        if self.embed is None:
            self.build(x.shape, x.device)
        for m in self.mha_layers:  # (lazily built layers: parameters created before a .to(device) of the parent are moved by it)
            if m.wqkv.weight.device != x.device:
                m.to(x.device)
        # kernel = stride = 4^p on NEST-ordered rows: the input is, without a copy, an (N M / 4^p) x (4^p Fin) matrix and the
        # embedding one GEMM against the [4^p Fin, d] view of the Conv1D weights (HealpyPseudoConv.forward)
        N, M, Fin = x.shape
        w2 = self.embed.weight.permute(2, 1, 0).reshape(g * Fin, self.embedding_size)  # row (i, f) <- weight[o, f, i]
        x = torch.addmm(self.embed.bias, x.reshape(N * (M // g), g * Fin), w2).reshape(N, M // g, self.embedding_size)
        if self.positional_encoding:
            x = self.pos_encoder(x)
        mask = self.mask if mask is None else mask  # (the call's mask overrides the constructor's)
        if mask is not None:  # checked and laid out once: the same operand goes to every block
            if self.mask is not None and mask is self.mask and mask.device != x.device:
                self.mask = mask = mask.to(x.device)
            mask = _dense_mask(mask, x.shape[0], self.num_heads, x.shape[1], x.device)
        for mha in self.mha_layers:
            x = mha(x, mask=mask)
        return x

    call = forward


__all__ = ["scaled_dot_product_attention", "scaled_dot_product_sparse_attention", "AddPositionEmbs", "MultiHeadAttention",
           "Graph_Transformer", "Graph_ViT", "neighbour_tables"]
