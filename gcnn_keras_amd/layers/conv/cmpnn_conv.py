"""CMPNN's communicate round (kgcnn/literature/CMPNN.py:126-150; Song et al. 2020) and its fused route on
csrc/mp_cmpnn.hip.

``CMPNNBoost`` is the node booster ``h' = h + pool(he) * max(he)`` (CMPNN.py:131-135; with ``m_only`` the product alone,
which the last step concatenates, CMPNN.py:148-150).  ``CMPNNCommunicate`` is one whole round: the booster, then the directed
edge update ``he' = act(Dense(h'[sender] - he[reverse]) + he0)`` (CMPNN.py:138-145) with the round's own
``Dense(**edge_dense)``.  Each has two routes:

* the *layer sequence*, the reference's ops on the engine's layers (two ``PoolingLocalEdges``, ``LazyMultiply``, ``LazyAdd``;
  ``GatherNodesOutgoing``, ``DMPNNGatherEdgesPairs``, ``LazySubtract``, ``Dense``, ``LazyAdd``, ``Activation``, ``Dropout``):
  every configuration, every call with keyword arguments and every tape;
* the *fused route*, two launches per round: ``mp_cmpnn_boost_f32`` walks each receiver's edge segment once for both
  reductions (equal bits with the four layers), ``mp_directed_edge_update_f32`` is a tiled FP32-MFMA GEMM that forms the
  difference of the two gathered rows while it stages them and applies bias, activation, residual and activation in its
  epilogue; the seven edge-sized intermediates are never written.

Served sizes (``fused_communicate_supported``, decided in ``build``): node width = edge width = ``edge_dense["units"]`` = a
multiple of 4, both activations among the engine's codes, sum or mean ``pooling_kwargs``, float32, ``use_bias`` either way.
The fused route is forward-only: in grad mode it steps aside when an input or a weight requires grad, and so do
``use_fused_communicate = False`` and keyword arguments.  Max pooling has no reverse rule, so a tape through a round raises
``NotImplementedError`` (``autograd.SegmentSum``).  Edge lists that are not receiver-sorted go through the plan's CSR
permutation.  The reverse position is shifted into the batch the way ``DMPNNGatherEdgesPairs`` does it, by an index plan over
the edge tensor, once per (pair tensor, edge partition).
"""
import torch

from ... import _ffi
from ..base import GraphBaseLayer
from ..gather import GatherNodesOutgoing
from ..modules import Activation, Dense, Dropout, LazyAdd, LazyMultiply, LazySubtract, _activation_name
from ..pooling import PoolingLocalEdges
from .dmpnn_conv import DMPNNGatherEdgesPairs

EDGE_TILE = _ffi.MP_CMPNN_EDGE_TILE    # edges per tile of mp_directed_edge_update_f32
_FUSED_POOLING = {"mean": _ffi.MP_MEAN, "segment_mean": _ffi.MP_MEAN, "reduce_mean": _ffi.MP_MEAN,
                  "sum": _ffi.MP_SUM, "segment_sum": _ffi.MP_SUM, "reduce_sum": _ffi.MP_SUM}


def fused_boost_supported(node_width, edge_width, pooling_method, dtype="float32"):
    """True when the booster with these sizes runs on ``mp_cmpnn_boost_f32``."""
    if node_width is None or edge_width is None or int(node_width) != int(edge_width) or int(node_width) < 4 \
            or int(node_width) % 4:
        return False
    if dtype not in ("float32", torch.float32):
        return False
    return pooling_method in _FUSED_POOLING


def fused_communicate_supported(node_width, edge_width, units, activation, edge_activation, pooling_method,
                                dtype="float32"):
    """True when one round with these sizes runs on the two kernels of csrc/mp_cmpnn.hip (the configuration decides)."""
    if not fused_boost_supported(node_width, edge_width, pooling_method, dtype):
        return False
    if units is None or int(units) != int(node_width):
        return False
    return _activation_name(activation) in _ffi.ACTIVATION_CODES and \
        _activation_name(edge_activation) in _ffi.ACTIVATION_CODES


def _check_sizes(what, h, he, plan):
    hv, ev = h.values, he.values
    _ffi.require_device(hv, ev)
    if hv.dtype != torch.float32 or ev.dtype != torch.float32 or hv.dim() != 2 or ev.dim() != 2:
        raise ValueError("%s expects float32 nodes (batch, [N], F) and edges (batch, [M], F)" % what)
    n, e, f = plan.N, plan.M, int(hv.shape[1])
    if plan.K != 2 or e != int(ev.shape[0]) or n != int(hv.shape[0]) or int(ev.shape[1]) != f:
        raise ValueError("%s: %d node rows of width %d and %d edge rows of width %d for %d nodes and %d edges of %d columns"
                         % (what, int(hv.shape[0]), f, int(ev.shape[0]), int(ev.shape[1]), n, e, plan.K))
    if n >= 2 ** 31 - 1 or e >= 2 ** 31 - EDGE_TILE:
        raise ValueError("%s indexes nodes and edges with 32 bits" % what)
    return n, e, f


def boost_values(h, he, edge_index, pool_op, m_only=False):
    """``h + pool(he) * max(he)`` per receiver (``m_only``: the product alone) on ``mp_cmpnn_boost_f32``."""
    plan = edge_index.index_plan(h)
    plan.validate()
    n, e, f = _check_sizes("the fused CMPNN booster", h, he, plan)
    ptr0, perm0, _ = plan.csr(0)
    hv, ev = h.values.detach().contiguous(), he.values.detach().contiguous()
    out = torch.empty((n, f), dtype=torch.float32, device=hv.device)
    _ffi.call("mp_cmpnn_boost_f32", _ffi.ptr(hv), _ffi.ptr(ev), e, f, _ffi.ptr(ptr0), _ffi.ptr(perm0), n, pool_op,
              1 if m_only else 0, _ffi.ptr(out), _ffi.stream())
    return h.with_values(out)


def reverse_positions(edges, reverse_pairs):
    """``(rev, flags)``: per edge the BATCH position of its reverse edge as int32, -1 where there is none, and the flag
    word of the index plan that shifted it (``DMPNNGatherEdgesPairs``' plan over the edge tensor).  Cached on the pair
    tensor per edge partition."""
    pairs = reverse_pairs.values
    key = ("reverse", edges.row_splits.data_ptr(), int(edges.values.shape[0]), pairs.data_ptr(), pairs._version)
    hit = reverse_pairs._plans.get(key)
    if hit is None:
        _ffi.require_device(pairs, edges.row_splits)
        if pairs.dtype != torch.int64 or pairs.dim() != 2 or int(pairs.shape[1]) != 1:
            raise ValueError("reverse edge positions must be int64 of shape (batch, [M], 1)")
        has_pair = pairs >= 0
        plan = reverse_pairs.with_values(torch.where(has_pair, pairs, torch.zeros_like(pairs))).index_plan(edges)
        plan.validate()
        rev = torch.where(has_pair[:, 0], plan.col(0), torch.full_like(plan.col(0), -1)).contiguous()
        hit = reverse_pairs._plans[key] = (rev, plan.flags)
    return hit


def directed_edge_update_values(h, he, he0, edge_index, reverse_pairs, kernel, bias, activation, edge_activation,
                                out=None):
    """``act2(act1((h[sender] - he[reverse]) W + b) + he0)`` on ``mp_directed_edge_update_f32``.  ``out`` (optional) is the
    values tensor to write; it must not share memory with ``he`` (``ValueError``)."""
    plan = edge_index.index_plan(h)
    plan.validate()
    n, e, f = _check_sizes("the fused directed edge update", h, he, plan)
    hv, ev, e0 = h.values.detach().contiguous(), he.values.detach().contiguous(), he0.values.detach().contiguous()
    _ffi.require_device(e0, kernel)
    if tuple(e0.shape) != (e, f) or e0.dtype != torch.float32 or tuple(kernel.shape) != (f, f):
        raise ValueError("the fused directed edge update: he0 %s and kernel %s for %d edges of width %d"
                         % (tuple(e0.shape), tuple(kernel.shape), e, f))
    if reverse_pairs.nrows() != he.nrows() or int(reverse_pairs.values.shape[0]) != e:
        raise ValueError("the fused directed edge update: %d reverse positions in %d lists for %d edges in %d lists"
                         % (int(reverse_pairs.values.shape[0]), reverse_pairs.nrows(), e, he.nrows()))
    rev, flags = reverse_positions(he, reverse_pairs)
    if out is None:
        out = torch.empty((e, f), dtype=torch.float32, device=hv.device)
    elif tuple(out.shape) != (e, f) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("the fused directed edge update writes a contiguous float32 (%d, %d) tensor" % (e, f))
    _ffi.call("mp_directed_edge_update_f32", _ffi.ptr(hv), n, _ffi.ptr(ev), _ffi.ptr(e0), e, f, _ffi.ptr(plan.col(1)),
              _ffi.ptr(rev), _ffi.ptr(kernel.detach()), _ffi.ptr(None if bias is None else bias.detach()),
              _ffi.activation_code(activation), _ffi.activation_code(edge_activation), 0.05, _ffi.ptr(out),
              _ffi.ptr(flags), _ffi.stream())
    return he.with_values(out)


class CMPNNBoost(GraphBaseLayer):
    r"""Node booster of CMPNN (kgcnn/literature/CMPNN.py:131-135): ``boost([h, he, edge_index])`` returns
    ``h + pool(he) * max(he)`` per receiver, with ``m_only=True`` the product ``m`` alone (CMPNN.py:148-150).
    ``use_fused_communicate`` (default True): sizes that fit ``fused_boost_supported`` run on ``mp_cmpnn_boost_f32`` outside
    a tape (``fused_communicate``, decided in ``build``)."""

    weight_gradients = True   # no weights; the four layers carry their rules (max pooling refuses a tape)

    def __init__(self, pooling_method="mean", pooling_index=0, m_only=False, **kwargs):
        super().__init__(**kwargs)
        self.pooling_method = pooling_method
        self.pooling_index = pooling_index
        self.m_only = bool(m_only)
        flags = dict(self._kgcnn_info)
        self.lay_pool = PoolingLocalEdges(pooling_method=pooling_method, pooling_index=pooling_index, **flags)
        self.lay_max = PoolingLocalEdges(pooling_method="segment_max")
        self.lay_mul = LazyMultiply()
        self.lay_add = LazyAdd()
        self.use_fused_communicate = True
        self.fused_communicate = None      # decided in build(): the sizes fit the fused kernel

    def build(self, input_shape):
        super().build(input_shape)
        plain = self.pooling_index == 0 and self.has_unconnected and not self.is_sorted
        self.fused_communicate = plain and fused_boost_supported(input_shape[0][-1], input_shape[1][-1],
                                                                 self.pooling_method, self.dtype)

    def layer_sequence(self, h, he, edge_index, **kwargs):
        """The reference's four layers."""
        m_pool = self.lay_pool([h, he, edge_index], **kwargs)
        m_max = self.lay_max([h, he, edge_index], **kwargs)
        m = self.lay_mul([m_pool, m_max], **kwargs)
        return m if self.m_only else self.lay_add([h, m], **kwargs)

    def call(self, inputs, **kwargs):
        """inputs: ``[h (batch,[N],F), he (batch,[M],F), edge_index (batch,[M],2)]`` -> ``(batch,[N],F)``."""
        h, he, edge_index = inputs
        if self.fused_communicate and self.use_fused_communicate and not kwargs:
            from ...autograd import needs_grad
            if not needs_grad(h.values, he.values):
                return boost_values(h, he, edge_index, _FUSED_POOLING[self.pooling_method], self.m_only)
        return self.layer_sequence(h, he, edge_index, **kwargs)

    def get_config(self):
        config = super().get_config()
        config.update({"pooling_method": self.pooling_method, "pooling_index": self.pooling_index, "m_only": self.m_only})
        return config


class CMPNNCommunicate(GraphBaseLayer):
    r"""One communicate round of CMPNN (kgcnn/literature/CMPNN.py:129-145) with its own ``Dense(**edge_dense)``:
    ``round([h, he, he0, edge_index, reverse_pairs])`` returns the updated ``(h, he)``.  ``use_fused_communicate`` (default
    True): sizes that fit ``fused_communicate_supported`` take the two kernels of csrc/mp_cmpnn.hip outside a tape
    (``fused_communicate``, decided in ``build``)."""

    # Dense, the gathers and the elementwise layers carry their rules; the max pooling of the booster refuses a tape
    # (autograd.SegmentSum), so a round never returns a silent zero gradient
    weight_gradients = True

    def __init__(self, edge_dense=None, edge_activation=None, pooling_kwargs=None, dropout=None, **kwargs):
        super().__init__(**kwargs)
        self.edge_dense = dict(edge_dense) if edge_dense is not None else {"units": 300, "activation": "linear"}
        self.edge_activation = dict(edge_activation) if edge_activation is not None else {"activation": "relu"}
        self.pooling_kwargs = dict(pooling_kwargs) if pooling_kwargs is not None else {"pooling_method": "sum"}
        self.dropout = dict(dropout) if dropout else None
        self.lay_boost = CMPNNBoost(**self.pooling_kwargs)
        self.pooling_method = self.lay_boost.pooling_method
        self.lay_gather_out = GatherNodesOutgoing()
        self.lay_gather_pairs = DMPNNGatherEdgesPairs()
        self.lay_subtract = LazySubtract()
        self.lay_dense = Dense(**self.edge_dense)
        self.lay_add = LazyAdd()
        self.lay_act = Activation(**self.edge_activation)
        self.lay_drop = Dropout(**self.dropout) if self.dropout else None
        self.use_fused_communicate = True
        self.fused_communicate = None      # decided in build(): the sizes fit the fused kernels

    def build(self, input_shape):
        """The round's Dense kernel (so ``set_weights`` works before a first call) and the route decision."""
        super().build(input_shape)
        fn, fe = input_shape[0][-1], input_shape[1][-1]
        self.lay_dense.ensure_built((None, None, int(fe)))
        self.lay_boost.ensure_built([input_shape[0], input_shape[1], input_shape[3]])
        self.fused_communicate = bool(self.lay_boost.fused_communicate and input_shape[2][-1] == fe and
                                      fused_communicate_supported(fn, fe, self.lay_dense.units, self.lay_dense.activation,
                                                                  self.lay_act.activation, self.pooling_method,
                                                                  self.dtype))

    def needs_grad(self, *inputs):
        """The kernels read the weights in place and have no reverse rule: any tape steps aside to the layer sequence."""
        from ...autograd import needs_grad
        return needs_grad(*inputs) or needs_grad(self.lay_dense.kernel, self.lay_dense.bias)

    def call(self, inputs, **kwargs):
        """inputs: ``[h (batch,[N],F), he (batch,[M],F), he0 (batch,[M],F), edge_index (batch,[M],2), reverse_pairs
        (batch,[M],1)]`` -> ``(h', he')``."""
        h, he, he0, edge_index, reverse_pairs = inputs
        if (self.fused_communicate and self.use_fused_communicate and not kwargs
                and not self.needs_grad(h.values, he.values, he0.values)):
            h = boost_values(h, he, edge_index, _FUSED_POOLING[self.pooling_method])
            he = directed_edge_update_values(h, he, he0, edge_index, reverse_pairs, self.lay_dense.kernel,
                                             self.lay_dense.bias, self.lay_dense.activation, self.lay_act.activation)
            return h, he
        h = self.lay_boost.layer_sequence(h, he, edge_index, **kwargs)
        h_out = self.lay_gather_out([h, edge_index], **kwargs)
        e_rev = self.lay_gather_pairs([he, reverse_pairs], **kwargs)
        he = self.lay_subtract([h_out, e_rev], **kwargs)
        he = self.lay_dense(he, **kwargs)
        he = self.lay_add([he, he0], **kwargs)
        he = self.lay_act(he, **kwargs)
        if self.lay_drop is not None:
            he = self.lay_drop(he, **kwargs)
        return h, he

    def get_config(self):
        config = super().get_config()
        config.update({"edge_dense": dict(self.edge_dense), "edge_activation": dict(self.edge_activation),
                       "pooling_kwargs": dict(self.pooling_kwargs), "dropout": dict(self.dropout) if self.dropout else None})
        return config
