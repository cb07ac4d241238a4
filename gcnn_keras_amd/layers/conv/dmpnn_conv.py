"""Directed message passing helpers of DMPNN (mirror of kgcnn/layers/conv/dmpnn_conv.py:9-89).

``DMPNNGatherEdgesPairs``: ``out[e] = edges[pair[e]]`` where ``pair[e]`` is the (per-graph) position of the reverse edge,
zeros where there is none (``pair[e] < 0``, dmpnn_conv.py:39-46).  ``DMPNNPPoolingEdgesDirected`` is the reference's
sequence (dmpnn_conv.py:83-87): sum the edge states at their receiver, gather that sum at each edge's sender, subtract the
state of the reverse edge.

``DMPNNStep`` (this engine's own layer; the reference spells the round inline, kgcnn/literature/DMPNN.py:136-142) is one
whole round with the model's shared ``Dense(**edge_dense)`` and ``Activation(**edge_activation)``:

    h'[e] = act2(act1((R[send e] - h[rev e]) W + b) + h0[e]),   R[n] = sum of h over the edges received by n

It has two routes:

* the *layer sequence*, today's ops (``DMPNNPPoolingEdgesDirected``, ``Dense``, ``LazyAdd``, ``Activation``): every
  configuration, every call with keyword arguments and every tape the fused rule does not serve;
* the *fused route*, two launches per round: ``mp_segment_reduce_csr_f32`` over the receiver CSR of the plan gives ``R``,
  ``mp_directed_edge_update_f32`` (csrc/mp_cmpnn.hip) does the rest; every round writes a fresh tensor.  On a tape
  (an input or the shared Dense requires grad) the same two launches run inside ``autograd.DirectedEdgeUpdate``, whose
  backward is csrc/mp_dmpnn.hip: served for ``act1 = linear`` and ``act2`` linear or relu, any other pair steps aside to
  the layer sequence.

Served sizes (``fused_step_supported``, decided in ``build``): the width of ``h`` = the width of ``h0`` = the Dense's units =
a multiple of 4, both activations among the engine's codes, float32.
"""
import torch

from ... import _ffi
from ..base import GraphBaseLayer
from ..gather import GatherNodesIngoing, GatherNodesOutgoing
from ..modules import Activation, Dense, LazyAdd, LazySubtract, _activation_name, binary_values
from ..pooling import PoolingLocalEdges

_TAPE_ACT1 = ("linear", None)            # mp_directed_edge_update_grad_f32 takes act2's derivative from the output
_TAPE_ACT2 = ("linear", None, "relu")


class DMPNNGatherEdgesPairs(GraphBaseLayer):

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.gather_layer = GatherNodesIngoing()

    def call(self, inputs, **kwargs):
        """inputs: ``[edges (batch,[M],F), pair_index (batch,[M],1) int64]`` -> ``(batch,[M],F)``."""
        edges, pair_index = inputs
        pairs = pair_index.values
        has_pair = pairs >= 0
        safe = pair_index.with_values(torch.where(has_pair, pairs, torch.zeros_like(pairs)))
        gathered = self.gather_layer([edges, safe], **kwargs)
        mask = has_pair.to(gathered.values.dtype).reshape((-1,) + (1,) * (gathered.values.dim() - 1))
        return gathered.with_values(binary_values(_ffi.MP_MUL, gathered.values, mask))


class DMPNNPPoolingEdgesDirected(GraphBaseLayer):

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.pool_edge_1 = PoolingLocalEdges(pooling_method="sum")
        self.gather_edges = GatherNodesOutgoing()
        self.gather_pairs = DMPNNGatherEdgesPairs()
        self.subtract_layer = LazySubtract()

    def call(self, inputs, **kwargs):
        """inputs: ``[nodes, edges (batch,[M],F), edge_index (batch,[M],2), edge_reverse_pair (batch,[M],1)]``."""
        nodes, edges, edge_index, reverse_pair = inputs
        received = self.pool_edge_1([nodes, edges, edge_index], **kwargs)
        at_sender = self.gather_edges([received, edge_index], **kwargs)
        return self.subtract_layer([at_sender, self.gather_pairs([edges, reverse_pair], **kwargs)], **kwargs)


def fused_step_supported(edge_width, initial_width, units, activation, edge_activation, dtype="float32"):
    """True when one round with these sizes runs on the fused route (the configuration decides)."""
    if edge_width is None or initial_width is None or units is None:
        return False
    f = int(edge_width)
    if int(initial_width) != f or int(units) != f or f < 4 or f % 4:
        return False
    if dtype not in ("float32", torch.float32):
        return False
    return _activation_name(activation) in _ffi.ACTIVATION_CODES and \
        _activation_name(edge_activation) in _ffi.ACTIVATION_CODES


def fused_step_tape_supported(activation, edge_activation):
    """True when ``autograd.DirectedEdgeUpdate`` has a reverse for this activation pair."""
    return _activation_name(activation) in _TAPE_ACT1 and _activation_name(edge_activation) in _TAPE_ACT2


def reverse_csr(edges, reverse_pairs):
    """``(ptr, perm)``: CSR over the reverse positions of ``cmpnn_conv.reverse_positions`` - segment ``e`` lists the edges
    that name ``e`` as their reverse, in edge order; edges without a reverse lie in the extra segment ``E``.  ``ptr`` has
    ``E + 2`` entries.  Cached on the pair tensor per edge partition."""
    from .cmpnn_conv import reverse_positions
    pairs = reverse_pairs.values
    key = ("reverse_csr", edges.row_splits.data_ptr(), int(edges.values.shape[0]), pairs.data_ptr(), pairs._version)
    hit = reverse_pairs._plans.get(key)
    if hit is None:
        rev, _ = reverse_positions(edges, reverse_pairs)
        e, dev = int(rev.shape[0]), rev.device
        ptr = torch.empty(e + 2, dtype=torch.int32, device=dev)
        perm = None
        seg = torch.where(rev >= 0, rev, torch.full_like(rev, e)).contiguous()
        if e > 0:
            nbytes = _ffi.workspace_bytes("mp_sort_workspace_bytes", e)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            seg_sorted = torch.empty(e, dtype=torch.int32, device=dev)
            perm = torch.empty(e, dtype=torch.int32, device=dev)
            _ffi.call("mp_sort_segments_i32", _ffi.ptr(seg), e, _ffi.ptr(seg_sorted), _ffi.ptr(perm), _ffi.ptr(ws),
                      nbytes, _ffi.stream())
            seg = seg_sorted
        _ffi.call("mp_csr_from_sorted_i32", _ffi.ptr(seg) if e > 0 else None, e, e + 1, _ffi.ptr(ptr), _ffi.stream())
        hit = reverse_pairs._plans[key] = (ptr, perm)
    return hit


class DirectedStepSpec:
    """The index side and the activation pair of one fused round, for ``autograd.DirectedEdgeUpdate``: ``forward`` is the
    fused route's two launches on values tensors, ``grad`` their reverse."""

    def __init__(self, nodes, h, edge_index, reverse_pairs, activation, edge_activation):
        self.nodes, self.h, self.edge_index, self.reverse_pairs = nodes, h, edge_index, reverse_pairs
        self.activation, self.edge_activation = _activation_name(activation), _activation_name(edge_activation)
        self.plan = edge_index.index_plan(nodes)
        self.plan.validate()
        hv = h.values
        _ffi.require_device(hv)
        if hv.dtype != torch.float32 or hv.dim() != 2 or int(hv.shape[0]) != self.plan.M or self.plan.K != 2:
            raise ValueError("the fused DMPNN round expects float32 edge states (batch, [M], F) over an edge index of two "
                             "columns, got %s for %d edges of %d columns" % (tuple(hv.shape), self.plan.M, self.plan.K))
        self.n, self.e, self.f = self.plan.N, self.plan.M, int(hv.shape[1])   # the edge kernel's guards check the rest

    def forward(self, hv, h0v, kernel, bias):
        """``(R, y)`` of the values ``hv`` and ``h0v`` (E, F)."""
        from ...ops.segment import _segment_reduce_raw
        from .cmpnn_conv import directed_edge_update_values
        ptr0, perm0, _ = self.plan.csr(0)
        r = _segment_reduce_raw(_ffi.MP_SUM, hv, ptr0, perm0, self.n)
        y = directed_edge_update_values(self.nodes.with_values(r), self.h.with_values(hv), self.h.with_values(h0v),
                                        self.edge_index, self.reverse_pairs, kernel, bias, self.activation,
                                        self.edge_activation)
        return r, y.values

    def grad(self, r, hv, y, kernel, g, want_h=True, want_w=True, want_b=True):
        """``(h_bar, p, W_bar, b_bar)`` of the upstream gradient ``g`` (E, F); ``p`` is the gradient of ``h0``."""
        from ...ops.segment import _segment_reduce_raw
        from .cmpnn_conv import reverse_positions
        if not fused_step_tape_supported(self.activation, self.edge_activation):
            raise NotImplementedError("the fused DMPNN round has a reverse for a linear Dense and a linear or relu "
                                      "activation, got %r / %r" % (self.activation, self.edge_activation))
        n, e, f, dev = self.n, self.e, self.f, g.device
        rev, flags = reverse_positions(self.h, self.reverse_pairs)
        p = torch.empty((e, f), dtype=torch.float32, device=dev)
        q = torch.empty((e, f), dtype=torch.float32, device=dev)
        _ffi.call("mp_directed_edge_update_grad_f32", _ffi.ptr(g), _ffi.ptr(y), e, f, _ffi.ptr(kernel),
                  _ffi.activation_code(self.edge_activation), _ffi.ptr(p), _ffi.ptr(q), _ffi.stream())
        w_bar = b_bar = h_bar = None
        if want_w or want_b:
            w_bar = torch.empty((f, f), dtype=torch.float32, device=dev)
            b_bar = torch.empty((f,), dtype=torch.float32, device=dev) if want_b else None
            ws, nbytes = _ffi.float_workspace("mp_directed_edge_wgrad_ws_bytes", e, f, device=dev, none_if_empty=True)
            _ffi.call("mp_directed_edge_wgrad_f32", _ffi.ptr(r), n, _ffi.ptr(hv), e, f, _ffi.ptr(self.plan.col(1)),
                      _ffi.ptr(rev), _ffi.ptr(p), _ffi.ptr(w_bar), _ffi.ptr(b_bar), _ffi.ptr(ws), nbytes,
                      _ffi.ptr(flags), _ffi.stream())
            if not want_w:
                w_bar = None
        if want_h:
            ptr1, perm1, _ = self.plan.csr(1)
            r_bar = _segment_reduce_raw(_ffi.MP_SUM, q, ptr1, perm1, n)          # adjoint of the sender gather
            rptr, rperm = reverse_csr(self.h, self.reverse_pairs)
            h_bar = torch.empty((e, f), dtype=torch.float32, device=dev)
            _ffi.call("mp_directed_edge_hgrad_f32", _ffi.ptr(r_bar), n, _ffi.ptr(q), e, f, _ffi.ptr(self.plan.col(0)),
                      _ffi.ptr(rptr), _ffi.ptr(rperm), _ffi.ptr(h_bar), _ffi.ptr(flags), _ffi.stream())
        return h_bar, p, w_bar, b_bar


class DMPNNStep(GraphBaseLayer):
    r"""One round of DMPNN (kgcnn/literature/DMPNN.py:136-140) around the model's shared layers:
    ``step([nodes, h, h0, edge_index, reverse_pairs])`` returns
    ``act2(act1((R[sender] - h[reverse]) W + b) + h0)`` with ``R`` the sum of ``h`` at the receiver.  ``nodes`` only
    supplies the node partition of the index plan, as in ``DMPNNPPoolingEdgesDirected``.  ``dense`` is the builder's one
    ``Dense(**edge_dense)`` and ``activation`` its ``Activation(**edge_activation)``: the step owns no kernel of its own.
    ``use_fused_step`` (default True): sizes that fit ``fused_step_supported`` take the fused route (``fused_step``,
    decided in ``build``); on a tape it records ``autograd.DirectedEdgeUpdate`` where the activation pair is served
    (``fused_step_tape``) and runs the layer sequence otherwise."""

    weight_gradients = True   # the fused rule returns W_bar / b_bar; the layers of the sequence carry their own rules

    def __init__(self, dense=None, activation=None, edge_dense=None, edge_activation=None, **kwargs):
        super().__init__(**kwargs)
        self.lay_dense = dense if dense is not None else Dense(**(edge_dense or {"units": 128, "activation": "linear"}))
        self.lay_act = activation if activation is not None else Activation(**(edge_activation or {"activation": "relu"}))
        self.lay_pool = DMPNNPPoolingEdgesDirected()
        self.lay_add = LazyAdd()
        self.use_fused_step = True
        self.fused_step = None          # decided in build(): the sizes fit the fused route
        self.fused_step_tape = None     # ... and the activation pair has a reverse

    def build(self, input_shape):
        """``input_shape``: ``[nodes, h (batch, None, F), h0 (batch, None, F), edge_index, reverse_pairs]``; builds the
        shared Dense if nobody has (so ``set_weights`` works before a first call) and decides the route."""
        super().build(input_shape)
        fe, f0 = input_shape[1][-1], input_shape[2][-1]
        self.lay_dense.ensure_built((None, None, int(fe)))
        self.fused_step = bool(fused_step_supported(fe, f0, self.lay_dense.units, self.lay_dense.activation,
                                                    self.lay_act.activation, self.dtype))
        self.fused_step_tape = bool(self.fused_step and fused_step_tape_supported(self.lay_dense.activation,
                                                                                  self.lay_act.activation))

    def layer_sequence(self, nodes, h, h0, edge_index, reverse_pairs, **kwargs):
        """The reference's layers."""
        m = self.lay_pool([nodes, h, edge_index, reverse_pairs], **kwargs)
        return self.lay_act(self.lay_add([self.lay_dense(m, **kwargs), h0], **kwargs), **kwargs)

    def call(self, inputs, **kwargs):
        """inputs: ``[nodes (batch,[N],...), h (batch,[M],F), h0 (batch,[M],F), edge_index (batch,[M],2), reverse_pairs
        (batch,[M],1)]`` -> ``(batch,[M],F)``."""
        nodes, h, h0, edge_index, reverse_pairs = inputs
        if self.fused_step and self.use_fused_step and not kwargs:
            from ...autograd import DirectedEdgeUpdate, needs_grad
            dense = self.lay_dense
            on_tape = needs_grad(h.values, h0.values, dense.kernel, dense.bias)
            if not on_tape or self.fused_step_tape:
                spec = DirectedStepSpec(nodes, h, edge_index, reverse_pairs, dense.activation, self.lay_act.activation)
                if on_tape:
                    return h.with_values(DirectedEdgeUpdate.apply(h.values, h0.values, dense.kernel, dense.bias, spec))
                return h.with_values(spec.forward(h.values.detach().contiguous(), h0.values.detach().contiguous(),
                                                  dense.kernel, dense.bias)[1])
        return self.layer_sequence(nodes, h, h0, edge_index, reverse_pairs, **kwargs)

    def get_config(self):
        config = super().get_config()
        config.update({"edge_dense": self.lay_dense.get_config(), "edge_activation": self.lay_act.get_config()})
        return config
