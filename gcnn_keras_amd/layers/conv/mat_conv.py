"""Layers of the Molecule Attention Transformer (mirror of kgcnn/layers/conv/mat_conv.py:7-185) on the engine.

The reference runs MAT on padded dense tensors: per head a ``(batch, Nmax, Nmax, units)`` score tensor, a ``-1/epsilon``
mask, a softmax over the sender axis, and padded distance and adjacency matrices.  Here the hot path stays ragged:
``MATAttentionHead([hn, xyz, edge_weight, edge_index])`` is three ``Dense`` launches and ONE ``mp_mat_attention_f32``
(csrc/mp_mat.hip, which states the algebra): every atom attends to every atom of its molecule, the distance term is formed
from the coordinates inside the kernel and the adjacency term is a walk over the receiver CSR of the index plan.  Padded
senders have weight exactly 0 in the reference (``exp(-1e7)`` underflows) and padded receivers are multiplied by 0, so the
ragged form computes the same numbers.

``FusedMATBlock`` runs one whole attention sub-block (all heads, the merging ``Dense`` and the residual) behind the layer
normalisation in TWO launches: one ``mp_dense_f32`` on the packed q|k|v kernel of all heads and ``mp_mat_attention_f32``
with the merge + residual epilogue.  Served sizes: ``FUSED_MAT_SIZES`` / ``fused_mat_supported``.

``MATDistanceMatrix``, ``MATReduceMask``, ``MATExpandMask``, ``MATGlobalPool`` on a padded tensor and
``CastEdgeIndicesToDenseAdjacency`` (layers/casting.py) exist for API compatibility and for tests: plain torch ops on
device tensors, off the hot path.

Inference only: dropout is the identity, and in grad mode (an input or weight that requires grad) both routes raise
``NotImplementedError`` - the pair attention has no reverse rule, and neither has ``GraphLayerNormalization``.
"""
import ctypes

import torch

from ... import _ffi
from ...ragged import RaggedTensor
from ..base import GraphBaseLayer, weight_epoch
from ..modules import Dense, dense_values

TRAFO_CODES = {None: _ffi.MP_MAT_TRAFO_NONE, "exp": _ffi.MP_MAT_TRAFO_EXP, "softmax": _ffi.MP_MAT_TRAFO_SOFTMAX}
MERGE_SUM_NAMES = ("add", "sum", "reduce_sum")   # kgcnn/literature/MAT.py:169; anything else concatenates

# csrc/mp_mat.hip, include/mpengine/mat.h: the tiles of the kernel and the caps of its merge epilogue
FUSED_MAT_SIZES = {"units_multiple": 4, "max_channels": _ffi.MP_MAT_EPILOGUE_MAX_CHANNELS,
                   "max_width": _ffi.MP_MAT_EPILOGUE_MAX_WIDTH,
                   "receiver_tile": _ffi.MP_MAT_RECV_TILE, "sender_tile": _ffi.MP_MAT_SEND_TILE}


def _raw(t):
    return ctypes.c_void_p(t.data_ptr())


def mat_attention_values(q, k, v, heads, units, xyz, node_splits, plan, weights, trafo, lambda_attention,
                         lambda_distance, lambda_adjacency, add_identity, merge_kernel=None, merge_sum=False,
                         residual=None):
    """``mp_mat_attention_f32`` on values tensors.  ``q, k, v``: ``(N, heads * units)`` float32, possibly column blocks
    of one wider tensor (last stride 1); ``weights`` ``(M,)`` or ``(M, 1)``; ``plan`` the index plan of the edges.
    Returns ``y (N, heads * units)``, or with ``merge_kernel`` ``residual + y @ merge_kernel`` ``(N, E)``."""
    _ffi.require_device(q, k, v, xyz, node_splits)
    n, c = int(q.shape[0]), heads * units
    for t in (q, k, v):
        if t.dtype != torch.float32 or t.dim() != 2 or tuple(t.shape) != (n, c) or (n > 0 and t.stride(1) != 1):
            raise ValueError("MAT attention: q, k, v must be float32 (N, %d) with unit column stride" % c)
    xyz = xyz.contiguous()
    if xyz.dtype != torch.float32 or tuple(xyz.shape) != (n, 3):
        raise ValueError("MAT attention: coordinates must be float32 (N, 3), got %s" % (tuple(xyz.shape),))
    if plan.K != 2 or plan.N != n:
        raise ValueError("MAT attention: the edge indices must be (batch, [M], 2) over the same %d atoms" % n)
    w = weights.contiguous().view(-1)
    if w.dtype != torch.float32 or int(w.shape[0]) != plan.M:
        raise ValueError("MAT attention: one float32 weight per edge, got %s for %d edges" % (tuple(weights.shape), plan.M))
    ptr0, perm0, _ = plan.csr(0)
    e, wm, res = 0, None, None
    if merge_kernel is not None:
        wm = merge_kernel.contiguous()
        e = int(wm.shape[1])
        res = None if residual is None else residual.contiguous()
    out = torch.empty((n, e if wm is not None else c), dtype=torch.float32, device=q.device)
    ld = lambda t: int(t.stride(0)) if n > 1 else c
    _ffi.call("mp_mat_attention_f32", _raw(q), ld(q), _raw(k), ld(k), _raw(v), ld(v), n, heads, units, _ffi.ptr(xyz),
              _ffi.ptr(node_splits), int(node_splits.shape[0]) - 1, _ffi.ptr(ptr0), _ffi.ptr(perm0),
              _ffi.ptr(plan.col(1)), _ffi.ptr(w), plan.M, TRAFO_CODES[trafo], float(lambda_attention),
              float(lambda_distance), float(lambda_adjacency), 1 if add_identity else 0, _ffi.ptr(wm), e,
              _ffi.MP_MAT_MERGE_SUM if merge_sum else _ffi.MP_MAT_MERGE_CONCAT, _ffi.ptr(res), _ffi.ptr(out),
              _ffi.ptr(plan.flags), _ffi.stream())
    return out


def _refuse_grad(*tensors):
    from ...autograd import needs_grad
    if needs_grad(*tensors):
        raise NotImplementedError("MAT: the all-pairs attention (and GraphLayerNormalization) has no reverse pass on the "
                                  "engine; call the model under torch.no_grad() with frozen weights")


class MATGlobalPool(GraphBaseLayer):
    """Masked sum over the atoms (mat_conv.py:7-28).  Ragged input: a segment sum over the rows of every molecule
    (``mp_pool_graph_f32``), one row per graph of the batch - a molecule without atoms gives zeros, as the padded sum
    does.  A padded ``(batch, N, F)`` tensor is summed over axis 1 by torch (compatibility, off the hot path)."""

    def __init__(self, pooling_method: str = "sum", **kwargs):
        super().__init__(**kwargs)
        self.pooling_method = pooling_method
        if self.pooling_method not in ["sum"]:
            raise ValueError("`pooling_method` must be in ['sum']")

    def call(self, inputs, mask=None, **kwargs):
        if not isinstance(inputs, RaggedTensor):
            return inputs.sum(dim=1)
        _ffi.require_device(inputs.values, inputs.row_splits)
        _refuse_grad(inputs.values)
        vals = inputs.values.contiguous()
        g, width = inputs.nrows(), int(vals.shape[1])
        out = torch.empty((g, width), dtype=torch.float32, device=vals.device)
        _ffi.call("mp_pool_graph_f32", _ffi.MP_SUM, _ffi.ptr(vals), _ffi.ptr(inputs.row_splits), g, max(width, 1), None,
                  _ffi.ptr(out), _ffi.stream())
        return out

    def get_config(self):
        config = super().get_config()
        config.update({"pooling_method": self.pooling_method})
        return config


class MATDistanceMatrix(GraphBaseLayer):
    """Padded distance matrix ``(batch, N, N, 1)`` and its mask from padded coordinates and their mask
    (mat_conv.py:31-67).  Compatibility layer: plain torch ops on device tensors, off the hot path - the ragged model never
    forms the matrix, ``MATAttentionHead`` takes this layer's ``trafo`` and the coordinates instead."""

    def __init__(self, trafo="exp", **kwargs):
        super().__init__(**kwargs)
        self.trafo = trafo
        if self.trafo not in [None, "exp", "softmax"]:
            raise ValueError("`trafo` must be in [None, 'exp', 'softmax']")

    def call(self, inputs, mask=None, **kwargs):
        diff = inputs.unsqueeze(1) - inputs.unsqueeze(2)
        dist = diff.square().sum(dim=-1, keepdim=True)
        dist_mask = (mask.unsqueeze(1) * mask.unsqueeze(2)).prod(dim=-1, keepdim=True)
        big = torch.ones_like(dist) / 1e-7     # ks.backend.epsilon()
        if self.trafo == "exp":
            dist = torch.exp(-(dist + torch.where(dist_mask.bool(), torch.zeros_like(dist), big)))
        elif self.trafo == "softmax":
            dist = torch.softmax(dist + torch.where(dist_mask.bool(), torch.zeros_like(dist), -big), dim=2)
        return dist * dist_mask, dist_mask

    def get_config(self):
        config = super().get_config()
        config.update({"trafo": self.trafo})
        return config


class MATReduceMask(GraphBaseLayer):
    """``reduce_prod`` of a mask over ``axis`` (mat_conv.py:70-87).  Compatibility layer: a torch op, off the hot path."""

    def __init__(self, axis: int, keepdims: bool, **kwargs):
        super().__init__(**kwargs)
        self.axis = axis
        self.keepdims = keepdims

    def call(self, inputs, **kwargs):
        return inputs.prod(dim=self.axis, keepdim=self.keepdims)

    def get_config(self):
        config = super().get_config()
        config.update({"axis": self.axis, "keepdims": self.keepdims})
        return config


class MATExpandMask(GraphBaseLayer):
    """``expand_dims`` of a mask (mat_conv.py:90-106).  Compatibility layer: a torch op, off the hot path."""

    def __init__(self, axis: int, **kwargs):
        super().__init__(**kwargs)
        self.axis = axis

    def call(self, inputs, **kwargs):
        return inputs.unsqueeze(self.axis)

    def get_config(self):
        config = super().get_config()
        config.update({"axis": self.axis})
        return config


class MATAttentionHead(GraphBaseLayer):
    r"""One attention head (mat_conv.py:109-185) on ragged inputs ``[hn, xyz, edge_weight, edge_index]``: node features
    ``(batch, [N], F)``, coordinates ``(batch, [N], 3)``, one weight per edge ``(batch, [M], 1)`` - the adjacency entries,
    duplicates add - and the edge indices ``(batch, [M], 2)`` (receiver, sender).  Returns ``(batch, [N], units)``:

    .. math::
        h'_i = \sum_{j \in mol(i)} (\lambda_a \, softmax_j(q_i k_j \sqrt{units}) + \lambda_d \, g(|r_i - r_j|^2)
        + \lambda_g (A_{ij} + \delta_{ij})) \, v_j

    channel by channel, as three ``Dense`` launches and one ``mp_mat_attention_f32``.  ``trafo`` (an attribute, not a
    constructor argument: the model builder copies it from its ``MATDistanceMatrix``) picks ``g``.  ``lambda_adjacency =
    None`` is ``1 - lambda_attention - lambda_distance``.  Dropout is the identity (inference)."""

    def __init__(self, units: int = 64, lambda_distance: float = 0.3, lambda_attention: float = 0.3,
                 lambda_adjacency=None, add_identity: bool = False, dropout=None, **kwargs):
        super().__init__(**kwargs)
        self.units = int(units)
        self.add_identity = bool(add_identity)
        self.lambda_distance = lambda_distance
        self.lambda_attention = lambda_attention
        if lambda_adjacency is not None:
            self.lambda_adjacency = lambda_adjacency
        else:
            self.lambda_adjacency = 1.0 - self.lambda_attention - self.lambda_distance
        self.scale = self.units ** -0.5
        self.dense_q = Dense(units=units)
        self.dense_k = Dense(units=units)
        self.dense_v = Dense(units=units)
        self._dropout = dropout
        self.trafo = "exp"
        self.use_fused_attention = True   # read by a FusedMATBlock that holds this head
        # engine.GraphedModel re-fills weight images of layers that carry `_packed` / `refresh_packed` before a replay:
        # the first head of a FusedMATBlock stands in for the block, which is no layer
        self._packed = None
        self._packed_block = None

    def refresh_packed(self):
        if self._packed_block is not None:
            self._packed_block.refresh_packed()

    def build(self, input_shape):
        super().build(input_shape)
        width = int(input_shape[0][-1])
        for lay in (self.dense_q, self.dense_k, self.dense_v):   # the reference's call order: the weight order
            lay.ensure_built((None, None, width))

    def signature(self):
        return (self.units, float(self.lambda_attention), float(self.lambda_distance), float(self.lambda_adjacency),
                self.add_identity, self.trafo, self.dtype)

    def weight_tensors(self):
        return [t for lay in (self.dense_q, self.dense_k, self.dense_v) for t in (lay.kernel, lay.bias)]

    def call(self, inputs, mask=None, **kwargs):
        if not all(isinstance(x, RaggedTensor) for x in inputs) or len(inputs) != 4:
            raise NotImplementedError("MATAttentionHead runs on ragged [nodes, coordinates, edge_weight, edge_index]; the "
                                      "padded form of the reference is not built")
        hn, xyz, weight, edge_index = inputs
        _refuse_grad(hn.values, xyz.values, weight.values, *self.weight_tensors())
        hv = hn.values
        q = dense_values(hv, self.dense_q.kernel, self.dense_q.bias)
        k = dense_values(hv, self.dense_k.kernel, self.dense_k.bias)
        v = dense_values(hv, self.dense_v.kernel, self.dense_v.bias)
        plan = edge_index.index_plan(hn)
        plan.validate()
        out = mat_attention_values(q, k, v, 1, self.units, xyz.values, hn.row_splits, plan, weight.values, self.trafo,
                                   self.lambda_attention, self.lambda_distance, self.lambda_adjacency, self.add_identity)
        return hn.with_values(out)

    def get_config(self):
        config = super().get_config()
        config.update({"units": self.units, "lambda_adjacency": self.lambda_adjacency,
                       "lambda_attention": self.lambda_attention, "lambda_distance": self.lambda_distance,
                       "dropout": self._dropout, "add_identity": self.add_identity})
        return config


def fused_mat_supported(units, num_heads, merge_units, dtype="float32", heads=None):
    """True when an attention sub-block with these sizes runs on the merge epilogue of csrc/mp_mat.hip; ``heads``: the
    block's head layers, which must share units, lambdas, ``add_identity`` and ``trafo``."""
    s = FUSED_MAT_SIZES
    if dtype not in ("float32", torch.float32):
        return False
    if units < 1 or units % s["units_multiple"] or num_heads < 1 or units * num_heads > s["max_channels"] \
            or not 1 <= merge_units <= s["max_width"]:
        return False
    if heads is not None:
        if len(heads) != num_heads or any(h.signature() != heads[0].signature() for h in heads[1:]):
            return False
    return True


class FusedMATBlock:
    """One attention sub-block of MAT behind its layer normalisation - ``heads`` ``MATAttentionHead`` layers over the same
    inputs, their merge (``merge_heads``: concatenated, or summed for "add" / "sum" / "reduce_sum"), the bias-free
    ``merge_dense`` and the residual - in two launches: ``mp_dense_f32`` on the packed ``(F, 3 H U)`` q|k|v kernel and bias
    of all heads, and ``mp_mat_attention_f32`` with the merge + residual epilogue.  ``block(hn, h, xyz, weight,
    edge_index)`` returns ``h + merge_dense(merge(heads(hn)))``.

    The packed image is rebuilt when ``weight_epoch()`` or a weight's version counter moves; for the same tensor objects
    it is re-filled in place, so a captured HIP graph reads the new weights (``refresh_packed``, called by
    ``engine.GraphedModel`` through the first head).  No host read-back: the block can be captured."""

    def __init__(self, heads, merge_dense, merge_heads="concat"):
        self.heads = list(heads)
        self.merge_dense = merge_dense
        self.merge_sum = merge_heads in MERGE_SUM_NAMES
        self._image = None          # (kernel (F, 3C), bias (3C))
        self._image_key = None      # (epoch, addresses, versions)
        self.heads[0]._packed_block = self

    def supported(self):
        """The configuration fits the kernel and every head's switch is on."""
        p = self.heads[0]
        return (all(h.use_fused_attention for h in self.heads) and self.merge_dense.bias is None
                and not self.merge_dense.use_bias and self.merge_dense.activation == "linear"
                and fused_mat_supported(p.units, len(self.heads), self.merge_dense.units, p.dtype, self.heads))

    def weight_tensors(self):
        return [t for h in self.heads for t in h.weight_tensors()] + [self.merge_dense.kernel]

    def route(self, hn, h, kwargs=None):
        """True when this call takes the fused kernels; raises in grad mode (MAT has no reverse on either route)."""
        _refuse_grad(hn.values, h.values, *self.weight_tensors())
        return (not kwargs and hn.values.dtype == torch.float32 and hn.values.dim() == 2 and self.supported())

    def _layers_in_order(self):
        return [lay for name in ("dense_q", "dense_k", "dense_v") for lay in (getattr(h, name) for h in self.heads)]

    def _packed_qkv(self):
        lays = self._layers_in_order()
        tensors = [t for lay in lays for t in (lay.kernel, lay.bias)]
        state = (tuple(t.data_ptr() for t in tensors), tuple(t._version for t in tensors))
        if self._image is not None and self._image_key == (weight_epoch(),) + state:
            return self._image
        kernel = torch.cat([lay.kernel.detach() for lay in lays], dim=1)
        bias = torch.cat([lay.bias.detach() for lay in lays], dim=0)
        if self._image is not None and self._image_key[1] == state[0] and self._image[0].shape == kernel.shape:
            self._image[0].copy_(kernel)     # same tensors, new values: in place, a captured graph reads this image
            self._image[1].copy_(bias)
        else:
            self._image = (kernel.contiguous(), bias.contiguous())
            # the marker engine.GraphedModel looks for; written past Layer.__setattr__, which would count the image as a
            # replaced weight and move the epoch under every other block's image
            self.heads[0].__dict__["_packed"] = self._image[0]
        self._image_key = (weight_epoch(),) + state
        return self._image

    def refresh_packed(self):
        if self._image is None:
            return
        lays = self._layers_in_order()
        if tuple(t.data_ptr() for lay in lays for t in (lay.kernel, lay.bias)) != self._image_key[1]:
            raise _ffi.EngineError("FusedMATBlock: q/k/v weight tensors were replaced after a graph capture; capture again")
        self._packed_qkv()

    def __call__(self, hn, h, xyz, weight, edge_index):
        p = self.heads[0]
        hv = hn.values
        _ffi.require_device(hv, edge_index.values)
        plan = edge_index.index_plan(hn)
        plan.validate()
        kernel, bias = self._packed_qkv()
        if int(hv.shape[1]) != int(kernel.shape[0]):
            raise ValueError("the heads were built for %d input columns, got %d" % (int(kernel.shape[0]), int(hv.shape[1])))
        c = p.units * len(self.heads)
        qkv = dense_values(hv, kernel, bias)
        out = mat_attention_values(qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:], len(self.heads), p.units, xyz.values,
                                   hn.row_splits, plan, weight.values, p.trafo, p.lambda_attention, p.lambda_distance,
                                   p.lambda_adjacency, p.add_identity, merge_kernel=self.merge_dense.kernel.detach(),
                                   merge_sum=self.merge_sum, residual=h.values)
        return h.with_values(out)
