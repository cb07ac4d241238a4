"""HamNet layers (mirror of kgcnn/layers/conv/hamnet_conv.py:12-544; Li et al., arXiv:2105.03688) on the engine.

``HamNaiveDynMessage`` is the message step: an attention over a receiver's edges whose logit reads the differences of the
end nodes' generalised momenta ``p`` and coordinates ``q`` and the edge row, and an edge update from ``[h_u || p_uv ||
q_uv || h_v]``.  ``HamNetFingerprintGenerator`` is the readout: a graph state, pooled from a Dense of the nodes, refined
``depth`` times by ``HamNetGlobalReadoutAttend`` (attention over the graph's nodes) and a GRU cell of its own per
iteration, with the layer's activation behind the cell.  ``HamNetGRUUnion`` / ``HamNetNaiveUnion`` merge an update into
the nodes or edges.

``call`` of every layer is the reference's op sequence on the engine's layers (the *layer sequence*: every configuration,
all training - every op carries its reverse rule, the GRU cells through ``autograd.GRUCombine``).  Outside a tape the
served sizes take fused routes (csrc/mp_hamnet.hip, which states the algebra):

* the message step: one node-side Dense launch (three when the edge update is asked for), ``mp_hamnet_edge_f32`` (per
  receiver-sorted position the difference row, the logit and the edge update; ``logit (E)`` and ``me (E, units_edge)`` are
  the only edge-sized tensors) and ``mp_hamnet_attend_f32`` (segment softmax, weighted sum of the senders' rows and the
  last activation per receiver);
* the fingerprint generator: ``1 + depth`` Dense launches and ``mp_hamnet_fingerprint_f32``, the loop over ``depth``
  inside the kernel.

The kernels read row-block views of the layers' own weights in place (nothing is repacked: a copy could go stale under
graph replay).  Served (``fused_hamnet_message_supported`` / ``fused_hamnet_fingerprint_supported``): float32; every
feature width a multiple of 4 up to 256; 1 to 8 coordinates; ``pooling_index == 0``; fingerprint ``depth`` up to 8 and
sum or mean start pooling.  Everything else, any call with keyword arguments and any call in grad mode where an input or a
weight requires grad takes the layer sequence, and so does ``use_fused_hamnet = False``.

Where this file leaves the reference's text: ``HamNaiveDynMessage.get_config`` also holds ``units_edge`` and
``HamNetFingerprintGenerator.get_config`` always holds ``rate``, ``noise_shape`` and ``seed`` (the reference's omits the
first and raises ``KeyError`` on the others without dropout, so neither round-trips there).
"""
import ctypes

import torch

from ... import _ffi
from ...ops.segment import reduce_op_code
from ..base import GraphBaseLayer
from ..gather import GatherEmbeddingSelection, GatherState
from ..modules import Activation, Dense, Dropout, LazyConcatenate, LazySubtract, _activation_name, dense_values
from ..pooling import PoolingLocalEdgesAttention, PoolingNodes, PoolingNodesAttention
from .attentivefp_conv import PoolingNodesAttentive, _GRUCell
from .mpnn_conv import GRUUpdate

_KERNEL_KEYS = ("kernel_regularizer", "activity_regularizer", "bias_regularizer", "kernel_constraint", "bias_constraint",
                "kernel_initializer", "bias_initializer")

FUSED_HAMNET_SIZES = {"max_width": _ffi.MP_HAMNET_MAX_WIDTH, "max_coords": _ffi.MP_HAMNET_MAX_COORDS,   # csrc/mp_hamnet.hip
                      "max_depth": _ffi.MP_HAMNET_MAX_DEPTH}

# Gated recurrent unit update (hamnet_conv.py:11-12): layers/conv/mpnn_conv.py
HamNetGRUUnion = GRUUpdate


def _width_ok(width):
    return width is not None and 4 <= int(width) <= FUSED_HAMNET_SIZES["max_width"] and int(width) % 4 == 0


def _acts_ok(*activations):
    return all(_activation_name(a) in _ffi.LAYER_ACTIVATION_CODES for a in activations)


def fused_hamnet_message_supported(units, units_edge, node_width, edge_width, coord_width, activation="kgcnn>leaky_relu",
                                   activation_last="elu", pooling_index=0, dtype="float32"):
    """True when a message step with these sizes runs on ``mp_hamnet_edge_f32`` / ``mp_hamnet_attend_f32`` (the
    configuration decides)."""
    if dtype not in ("float32", torch.float32) or pooling_index != 0:
        return False
    if not all(_width_ok(w) for w in (units, units_edge, node_width, edge_width)):
        return False
    if coord_width is None or not 1 <= int(coord_width) <= FUSED_HAMNET_SIZES["max_coords"]:
        return False
    return _acts_ok(activation, activation_last)


def fused_hamnet_fingerprint_supported(units, units_attend, node_width, depth=4, pooling_method="mean",
                                       activation="kgcnn>leaky_relu", recurrent_activation="sigmoid", dtype="float32"):
    """True when a fingerprint generator with these sizes runs on ``mp_hamnet_fingerprint_f32``."""
    if dtype not in ("float32", torch.float32):
        return False
    if not all(_width_ok(w) for w in (units, units_attend, node_width)):
        return False
    if not 0 <= int(depth) <= FUSED_HAMNET_SIZES["max_depth"]:
        return False
    try:
        if reduce_op_code(pooling_method) not in (_ffi.MP_SUM, _ffi.MP_MEAN):
            return False
    except (TypeError, ValueError, KeyError):
        return False
    return _acts_ok(activation, recurrent_activation)


def _needs_grad(layer, *values):
    from ...autograd import needs_grad
    return needs_grad(*values) or needs_grad(*[t for _, t in layer.weights])


def _det(t):
    return None if t is None else t.detach()


class HamNetNaiveUnion(GraphBaseLayer):
    r"""Union of a feature tensor and its update (hamnet_conv.py:15-98): :math:`x' = \sigma([x || x_u] W + b)`.
    ``use_fused_hamnet`` is carried for the model's switch; the layer is one concatenation and one Dense either way."""

    weight_gradients = True   # LazyConcatenate and Dense carry their rules

    def __init__(self, units: int, activation="kgcnn>leaky_relu", use_bias: bool = True,
                 kernel_initializer="glorot_uniform", bias_initializer="zeros", kernel_regularizer=None,
                 bias_regularizer=None, activity_regularizer=None, kernel_constraint=None, bias_constraint=None, **kwargs):
        super().__init__(**kwargs)
        self.units = int(units)
        self.use_bias = use_bias
        local = locals()
        kernel_args = {key: local[key] for key in _KERNEL_KEYS}
        self.lay_dense = Dense(units=units, activation=activation, use_bias=use_bias, **kernel_args)
        self.lay_concat = LazyConcatenate()
        self.use_fused_hamnet = True

    def build(self, input_shape):
        """``input_shape``: ``[x (batch, None, F), x_u (batch, None, Fu)]``."""
        super().build(input_shape)
        self.lay_dense.ensure_built((None, None, int(input_shape[0][-1]) + int(input_shape[1][-1])))

    def call(self, inputs, **kwargs):
        """inputs: ``[x (batch,[N],F), x_u (batch,[N],Fu)]`` -> ``(batch,[N],units)``."""
        n, nu = inputs
        return self.lay_dense(self.lay_concat([n, nu], **kwargs), **kwargs)

    def get_config(self):
        config = super().get_config()
        config.update({"units": self.units, "use_bias": self.use_bias})
        sub = self.lay_dense.get_config()
        config.update({key: sub[key] for key in _KERNEL_KEYS + ("use_bias", "activation")})
        return config


class HamNetGlobalReadoutAttend(GraphBaseLayer):
    r"""Attentive state update of the fingerprint generator (hamnet_conv.py:101-223): :math:`h'_i = \sigma(h_i W)`,
    :math:`a_i = w^T [s || h_i]`, :math:`m = \sigma_{last}(\sum_i \text{softmax}_i(a_i) h'_i)`; returns ``(m, a)``.  The
    layer has no launch of its own: inside ``HamNetFingerprintGenerator`` its weights are read by
    ``mp_hamnet_fingerprint_f32``; ``use_fused_hamnet`` is carried for the model's switch."""

    weight_gradients = True   # Dense, GatherState, LazyConcatenate, the attention pooling and Activation carry their rules

    def __init__(self, units, activation="kgcnn>leaky_relu", activation_last="elu", use_bias=True, kernel_regularizer=None,
                 bias_regularizer=None, activity_regularizer=None, kernel_constraint=None, bias_constraint=None,
                 kernel_initializer="glorot_uniform", bias_initializer="zeros", use_dropout=False, rate=None,
                 noise_shape=None, seed=None, **kwargs):
        super().__init__(**kwargs)
        self.units = int(units)
        self.use_bias = use_bias
        self.use_dropout = use_dropout
        local = locals()
        kernel_args = {key: local[key] for key in _KERNEL_KEYS}
        self.gather_state = GatherState()
        if self.use_dropout:
            self.dropout_layer = Dropout(rate=rate, noise_shape=noise_shape, seed=seed)
        self.dense_attend = Dense(units=units, activation=activation, use_bias=use_bias, **kernel_args)
        self.dense_align = Dense(1, activation="linear", use_bias=use_bias, **kernel_args)
        self.lay_concat = LazyConcatenate(axis=-1)
        self.pool_attention = PoolingNodesAttention()
        self.final_activ = Activation(activation=activation_last, activity_regularizer=activity_regularizer)
        self.use_fused_hamnet = True

    def build(self, input_shape):
        """``input_shape``: ``[state (batch, S), nodes (batch, None, F)]``; creates the weights in call order."""
        super().build(input_shape)
        s, f = int(input_shape[0][-1]), int(input_shape[1][-1])
        self.dense_attend.ensure_built((None, None, f))
        self.dense_align.ensure_built((None, None, s + f))

    def call(self, inputs, **kwargs):
        """inputs: ``[state (batch, S), nodes (batch,[N],F)]`` -> ``(m (batch, units), a (batch,[N],1))``."""
        hm_ftr, hv_ftr = inputs
        hm_v_ftr = self.gather_state([hm_ftr, hv_ftr], **kwargs)
        attend_ftr = hv_ftr
        if self.use_dropout:
            attend_ftr = self.dropout_layer(attend_ftr, **kwargs)
        attend_ftr = self.dense_attend(attend_ftr, **kwargs)
        align_ftr = self.lay_concat([hm_v_ftr, hv_ftr], **kwargs)
        if self.use_dropout:
            align_ftr = self.dropout_layer(align_ftr, **kwargs)
        align_ftr = self.dense_align(align_ftr, **kwargs)
        mm_ftr = self.pool_attention([attend_ftr, align_ftr], **kwargs)
        mm_ftr = self.final_activ(mm_ftr, **kwargs)
        return mm_ftr, align_ftr

    def get_config(self):
        config = super().get_config()
        config.update({"use_bias": self.use_bias, "units": self.units, "use_dropout": self.use_dropout})
        sub = self.dense_attend.get_config()
        config.update({key: sub[key] for key in _KERNEL_KEYS + ("activation",)})
        if self.use_dropout:
            drop = self.dropout_layer.get_config()
            config.update({key: drop[key] for key in ("rate", "noise_shape", "seed")})
        config.update({"activation_last": self.final_activ.get_config()["activation"]})
        return config


class HamNetFingerprintGenerator(GraphBaseLayer):
    r"""Fingerprint generator of HamNet (hamnet_conv.py:226-388): :math:`s^0 = \text{pool}(\sigma(h W))`, then ``depth``
    times :math:`m = f_l(s, h)` (``HamNetGlobalReadoutAttend``, its own weights per iteration) and
    :math:`s = \sigma(\text{GRU}_l(m, s))`.  Returns ``(batch, units)`` with ``PoolingNodes``' row count: trailing empty
    graphs are dropped, interior ones run the recurrence on ``elu(0)``.  Only the Keras default cell is built
    (``reset_after=True``, no ``dropout`` / ``recurrent_dropout``).  ``use_fused_hamnet`` (default True): sizes that fit
    ``fused_hamnet_fingerprint_supported`` run on ``mp_hamnet_fingerprint_f32`` outside a tape."""

    weight_gradients = True   # Dense, PoolingNodes, the readout layers and the GRU cells carry their rules

    def __init__(self, units: int, units_attend: int, activation="kgcnn>leaky_relu", use_bias: bool = True, depth=4,
                 pooling_method="mean", kernel_regularizer=None, bias_regularizer=None, activity_regularizer=None,
                 kernel_constraint=None, bias_constraint=None, kernel_initializer="glorot_uniform",
                 bias_initializer="zeros", recurrent_activation="sigmoid", recurrent_initializer="orthogonal",
                 recurrent_regularizer=None, recurrent_constraint=None, dropout=0.0, recurrent_dropout=0.0,
                 reset_after=True, use_dropout=False, rate=None, noise_shape=None, seed=None, **kwargs):
        super().__init__(**kwargs)
        if not reset_after or dropout or recurrent_dropout:
            raise NotImplementedError("HamNetFingerprintGenerator is built for the Keras default cell: reset_after=True, "
                                      "no dropout")
        self.units = int(units)
        self.units_attend = int(units_attend)
        self.use_bias = bool(use_bias)
        self.use_dropout = use_dropout
        self.depth = int(depth)
        self.pooling_method = pooling_method
        self._drop_conf = {"rate": rate, "noise_shape": noise_shape, "seed": seed}
        local = locals()
        kernel_args = {key: local[key] for key in _KERNEL_KEYS}
        self._gru_conf = {"recurrent_activation": recurrent_activation, "use_bias": use_bias,
                          "kernel_initializer": kernel_initializer, "recurrent_initializer": recurrent_initializer,
                          "bias_initializer": bias_initializer, "recurrent_regularizer": recurrent_regularizer,
                          "recurrent_constraint": recurrent_constraint, "dropout": dropout,
                          "recurrent_dropout": recurrent_dropout, "reset_after": reset_after}
        self.pool_nodes = PoolingNodes(pooling_method=self.pooling_method)
        self.vertex2mol = Dense(units=units, activation=activation, use_bias=use_bias, **kernel_args)
        self.readouts = [HamNetGlobalReadoutAttend(units=units_attend, activation=activation, activation_last="elu",
                                                   use_bias=use_bias, use_dropout=use_dropout, rate=rate,
                                                   noise_shape=noise_shape, seed=seed, **kernel_args)
                         for _ in range(self.depth)]
        self.unions = [_GRUCell(units, self._gru_conf) for _ in range(self.depth)]
        for i, cell in enumerate(self.unions):
            cell.name = "gru_cell" if i == 0 else "gru_cell_%d" % i
        self.final_activ = Activation(activation=activation, activity_regularizer=activity_regularizer)
        self.use_fused_hamnet = True

    def sublayers(self):
        """The weight order is the order in which ``call`` builds them: the start Dense, then readout and cell of each
        iteration in turn."""
        out = [self.pool_nodes, self.vertex2mol]
        for readout, cell in zip(self.readouts, self.unions):
            out += [readout, cell]
        return out + [self.final_activ]

    def build(self, input_shape):
        """``input_shape``: nodes ``(batch, None, F)``; creates every weight in the order of the layer sequence."""
        super().build(input_shape)
        f = int(input_shape[-1])
        self.vertex2mol.ensure_built((None, None, f))
        for readout, cell in zip(self.readouts, self.unions):
            readout.ensure_built([(None, self.units), (None, None, f)])
            cell.ensure_built((None, self.units_attend))

    def fused_supported(self, node_width):
        return fused_hamnet_fingerprint_supported(self.units, self.units_attend, node_width, self.depth,
                                                  self.pooling_method, self.vertex2mol.activation,
                                                  self._gru_conf["recurrent_activation"], self.dtype)

    def _call_fused(self, node):
        vals = node.values.detach().contiguous()
        _ffi.require_device(vals, node.row_splits)
        n, g, f, u, ua = int(vals.shape[0]), node.nrows(), int(vals.shape[1]), self.units, self.units_attend
        act = self.vertex2mol.activation
        v2m = self.vertex2mol
        if tuple(v2m.kernel.shape) != (f, u):
            raise ValueError("the fingerprint generator was built for another node width than %d" % f)
        m = dense_values(vals, _det(v2m.kernel), _det(v2m.bias), act) if n > 0 else None
        keep, cols = [], {key: [] for key in ("T", "w", "b", "K", "R", "b_in", "b_rec")}
        for readout, cell in zip(self.readouts, self.unions):
            att, ali = readout.dense_attend, readout.dense_align
            t = dense_values(vals, _det(att.kernel), _det(att.bias), att.activation) if n > 0 else None
            bias = _det(cell.bias)
            row = {"T": t, "w": _det(ali.kernel), "b": _det(ali.bias), "K": _det(cell.kernel),
                   "R": _det(cell.recurrent_kernel), "b_in": None if bias is None else bias[0],
                   "b_rec": None if bias is None else bias[1]}
            keep.append(row)                     # a pointer alone keeps no tensor alive
            for key, tensor in row.items():
                p = _ffi.ptr(tensor)
                cols[key].append(None if p is None else p.value)
        arr = lambda key: (ctypes.c_void_p * max(self.depth, 1))(*cols[key])
        cell0 = self.unions[0] if self.unions else None
        gru_act = cell0.act if cell0 is not None else _ffi.activation_code("tanh")
        rec_act = cell0.rec_act if cell0 is not None else _ffi.activation_code(self._gru_conf["recurrent_activation"])
        last = self.readouts[0].final_activ.activation if self.readouts else "elu"
        out = torch.empty((g, u), dtype=torch.float32, device=vals.device)
        term = torch.empty((max(n, 1),), dtype=torch.float64, device=vals.device)   # the kernel's node-sized workspace
        _ffi.call("mp_hamnet_fingerprint_f32", _ffi.ptr(vals), _ffi.ptr(m), n, _ffi.ptr(node.row_splits), g, f, u, ua,
                  self.depth, reduce_op_code(self.pooling_method), arr("T"), arr("w"), arr("b"), arr("K"), arr("R"),
                  arr("b_in"), arr("b_rec"), _ffi.activation_code(act), 0.05, _ffi.activation_code(last), gru_act,
                  rec_act, _ffi.ptr(term), _ffi.ptr(out), _ffi.stream())
        return out

    def call(self, inputs, **kwargs):
        """inputs: nodes ``(batch, [N], F)`` -> ``(batch, units)``."""
        node = PoolingNodesAttentive._without_trailing_empty(self.assert_ragged_input_rank(inputs))
        if (not kwargs and self.use_fused_hamnet and node.values.dtype == torch.float32 and node.values.dim() == 2
                and self.fused_supported(int(node.values.shape[1])) and not _needs_grad(self, node.values)):
            return self._call_fused(node)
        hv_ftr = node
        hm_ftr = self.vertex2mol(hv_ftr, **kwargs)
        hm_ftr = self.pool_nodes(hm_ftr, **kwargs)
        for readout, cell in zip(self.readouts, self.unions):
            mm_ftr, _ = readout([hm_ftr, hv_ftr], **kwargs)
            hm_ftr = cell([mm_ftr, hm_ftr], **kwargs)
            hm_ftr = self.final_activ(hm_ftr, **kwargs)
        return hm_ftr

    def get_config(self):
        config = super().get_config()
        config.update({"use_bias": self.use_bias, "units": self.units, "units_attend": self.units_attend,
                       "use_dropout": self.use_dropout, "depth": self.depth, "pooling_method": self.pooling_method})
        sub = self.vertex2mol.get_config()
        config.update({key: sub[key] for key in _KERNEL_KEYS + ("activation",)})
        config.update({key: self._gru_conf[key] for key in ("recurrent_activation", "recurrent_initializer",
                                                            "recurrent_regularizer", "recurrent_constraint", "dropout",
                                                            "recurrent_dropout", "reset_after")})
        config.update(self._drop_conf)
        return config


class HamNaiveDynMessage(GraphBaseLayer):
    r"""Message step of HamNet (hamnet_conv.py:391-544).  With :math:`p_{ij} = p_j - p_i`, :math:`q_{ij} = q_j - q_i`:
    :math:`a_{ij} = w^T [p_{ij} || q_{ij} || \epsilon_{ij}]`, :math:`m_i = \sigma_{last}(\sum_j \text{softmax}_j(a_{ij})
    \sigma(h_j W))` and :math:`m_{ij} = \sigma([h_i || p_{ij} || q_{ij} || h_j] W_e)`; returns ``(m_v, m_e)``.
    ``use_fused_hamnet`` (default True): sizes that fit ``fused_hamnet_message_supported`` run on the fused kernels
    outside a tape.  ``return_edge_update = False`` (set by the model on a round whose edge update nobody reads) returns
    ``m_e = None`` on either route and leaves ``dense_e`` out of the call."""

    # no weight is left off the tape: Dense, the gathers, LazySubtract, LazyConcatenate, Activation and the attention
    # pooling carry their rules
    weight_gradients = True

    def __init__(self, units, units_edge, activation="kgcnn>leaky_relu", activation_last="elu", use_bias=True,
                 kernel_regularizer=None, bias_regularizer=None, activity_regularizer=None, kernel_constraint=None,
                 bias_constraint=None, kernel_initializer="glorot_uniform", bias_initializer="zeros", use_dropout=False,
                 rate=None, noise_shape=None, seed=None, **kwargs):
        super().__init__(**kwargs)
        self.units = int(units)
        self.units_edge = int(units_edge)
        self.use_bias = use_bias
        self.use_dropout = use_dropout
        local = locals()
        kernel_args = {key: local[key] for key in _KERNEL_KEYS}
        self.gather_v = GatherEmbeddingSelection(selection_index=[0, 1])
        self.gather_p = GatherEmbeddingSelection(selection_index=[0, 1])
        self.gather_q = GatherEmbeddingSelection(selection_index=[0, 1])
        self.lazy_sub_p = LazySubtract()
        self.lazy_sub_q = LazySubtract()
        self.lay_concat_align = LazyConcatenate(axis=-1)
        self.lay_concat_edge = LazyConcatenate(axis=-1)
        if self.use_dropout:
            self.dropout_layer = Dropout(rate=rate, noise_shape=noise_shape, seed=seed)
        self.dense_attend = Dense(units=units, use_bias=use_bias, activation=activation, **kernel_args)
        self.dense_align = Dense(1, activation="linear", use_bias=use_bias, **kernel_args)
        self.dense_e = Dense(units=units_edge, activation=activation, use_bias=use_bias, **kernel_args)
        self.pool_attention = PoolingLocalEdgesAttention()
        self.final_activ = Activation(activation=activation_last, activity_regularizer=activity_regularizer)
        self.use_fused_hamnet = True
        self.return_edge_update = True

    def build(self, input_shape):
        """``input_shape``: ``[nodes (batch, None, F), edges (batch, None, D), p (batch, None, C), q (batch, None, C),
        edge_index]``; creates every weight in call order (the fused route reads the kernels directly)."""
        super().build(input_shape)
        f, d = int(input_shape[0][-1]), int(input_shape[1][-1])
        cp, cq = int(input_shape[2][-1]), int(input_shape[3][-1])
        self.dense_attend.ensure_built((None, None, f))
        self.dense_align.ensure_built((None, None, cp + cq + d))
        self.dense_e.ensure_built((None, None, 2 * f + cp + cq))

    def fused_supported(self, node_width, edge_width, coord_width):
        """The configuration fits the fused kernels."""
        pool = self.pool_attention
        return (bool(pool.has_unconnected)
                and fused_hamnet_message_supported(self.units, self.units_edge, node_width, edge_width, coord_width,
                                                   self.dense_attend.activation, self.final_activ.activation,
                                                   pool.pooling_index, self.dtype))

    def _route_fused(self, hv, he, p, q, kwargs):
        """True when this call takes the fused kernels."""
        if kwargs or not self.use_fused_hamnet:
            return False
        vals = [x.values for x in (hv, he, p, q)]
        if any(v.dtype != torch.float32 or v.dim() != 2 for v in vals):
            return False
        if vals[2].shape[1] != vals[3].shape[1]:
            return False
        if not self.fused_supported(int(vals[0].shape[1]), int(vals[1].shape[1]), int(vals[2].shape[1])):
            return False
        return not _needs_grad(self, *vals)

    def _call_fused(self, hv, he, p, q, edi):
        hvv, gv = hv.values.detach().contiguous(), he.values.detach().contiguous()
        pv, qv = p.values.detach().contiguous(), q.values.detach().contiguous()
        _ffi.require_device(hvv, gv, pv, qv, edi.values)
        plan = edi.index_plan(hv)
        plan.validate()
        n, e, u, ue = plan.N, plan.M, self.units, self.units_edge
        f, d, c = int(hvv.shape[1]), int(gv.shape[1]), int(pv.shape[1])
        if plan.K != 2 or n >= 2 ** 31 - 1 or e >= 2 ** 31 - 32:
            raise ValueError("the fused HamNet message takes (batch, [M], 2) indices of fewer than 2^31 nodes and edges")
        if int(gv.shape[0]) != e or int(pv.shape[0]) != n or int(qv.shape[0]) != n or int(hvv.shape[0]) != n:
            raise ValueError("the fused HamNet message: %d edge rows for %d edges, %d / %d / %d node rows for %d nodes"
                             % (int(gv.shape[0]), e, int(hvv.shape[0]), int(pv.shape[0]), int(qv.shape[0]), n))
        att, ali, den = self.dense_attend, self.dense_align, self.dense_e
        we = _det(den.kernel)
        if tuple(att.kernel.shape) != (f, u) or tuple(ali.kernel.shape) != (2 * c + d, 1) or \
                tuple(we.shape) != (2 * f + 2 * c, ue):
            raise ValueError("the message layer was built for other input widths than (%d nodes, %d edges, %d coordinates)"
                             % (f, d, c))
        want_me = bool(self.return_edge_update)
        mv = torch.empty((n, u), dtype=torch.float32, device=hvv.device)
        me = torch.empty((e, ue), dtype=torch.float32, device=hvv.device) if want_me else None
        if n > 0:
            t = dense_values(hvv, _det(att.kernel), _det(att.bias), att.activation)
            a = b = None
            if want_me and e > 0:
                # row blocks of dense_e.kernel, read in place (views: a repacked copy could go stale under replay)
                a = dense_values(hvv, we[:f], None, "linear")
                b = dense_values(hvv, we[f + 2 * c:], None, "linear")
            ptr0, perm0, _ = plan.csr(0)
            logit = torch.empty((max(e, 1),), dtype=torch.float32, device=hvv.device)
            _ffi.call("mp_hamnet_edge_f32", _ffi.ptr(a), _ffi.ptr(b), n, ue, _ffi.ptr(pv), _ffi.ptr(qv), c, _ffi.ptr(gv), d,
                      _ffi.ptr(_det(ali.kernel)), _ffi.ptr(_det(ali.bias)), _ffi.ptr(we[f:f + 2 * c]),
                      _ffi.ptr(_det(den.bias)), _ffi.ptr(plan.cols), e, _ffi.ptr(perm0), _ffi.activation_code(den.activation),
                      0.05, _ffi.ptr(logit), _ffi.ptr(me if e > 0 else None), _ffi.stream())
            _ffi.call("mp_hamnet_attend_f32", u, _ffi.ptr(t), _ffi.ptr(logit), n, _ffi.ptr(plan.cols), e, _ffi.ptr(ptr0),
                      _ffi.ptr(perm0), _ffi.activation_code(self.final_activ.activation), 0.05, _ffi.ptr(mv),
                      _ffi.stream())
        return hv.with_values(mv), (he.with_values(me) if want_me else None)

    def call(self, inputs, **kwargs):
        """inputs: ``[nodes (batch,[N],F), edges (batch,[M],D), p (batch,[N],C), q (batch,[N],C), edge_index
        (batch,[M],2)]`` -> ``(m_v (batch,[N],units), m_e (batch,[M],units_edge))``."""
        hv_ftr, he_ftr, p_ftr, q_ftr, edi = inputs
        if self._route_fused(hv_ftr, he_ftr, p_ftr, q_ftr, kwargs):
            return self._call_fused(hv_ftr, he_ftr, p_ftr, q_ftr, edi)
        if self.use_dropout:
            hv_ftr = self.dropout_layer(hv_ftr, **kwargs)
            he_ftr = self.dropout_layer(he_ftr, **kwargs)
        hv_u_ftr, hv_v_ftr = self.gather_v([hv_ftr, edi], **kwargs)
        q_u_ftr, q_v_ftr = self.gather_p([q_ftr, edi], **kwargs)
        p_u_ftr, p_v_ftr = self.gather_q([p_ftr, edi], **kwargs)
        p_uv_ftr = self.lazy_sub_p([p_v_ftr, p_u_ftr])   # LazySubtract hands keyword arguments on to the subtraction
        q_uv_ftr = self.lazy_sub_p([q_v_ftr, q_u_ftr])

        attend_ftr = self.dense_attend(hv_v_ftr, **kwargs)

        align_ftr = self.lay_concat_align([p_uv_ftr, q_uv_ftr, he_ftr], **kwargs)
        align_ftr = self.dense_align(align_ftr, **kwargs)
        mv_ftr = self.pool_attention([hv_ftr, attend_ftr, align_ftr, edi], **kwargs)
        mv_ftr = self.final_activ(mv_ftr, **kwargs)

        if not self.return_edge_update:
            return mv_ftr, None
        me_ftr = self.lay_concat_edge([hv_u_ftr, p_uv_ftr, q_uv_ftr, hv_v_ftr], **kwargs)
        me_ftr = self.dense_e(me_ftr)
        return mv_ftr, me_ftr

    def get_config(self):
        config = super().get_config()
        config.update({"use_bias": self.use_bias, "units": self.units, "units_edge": self.units_edge,
                       "use_dropout": self.use_dropout})
        sub = self.dense_attend.get_config()
        config.update({key: sub[key] for key in _KERNEL_KEYS + ("activation",)})
        if self.use_dropout:
            drop = self.dropout_layer.get_config()
            config.update({key: drop[key] for key in ("rate", "noise_shape", "seed")})
        config.update({"activation_last": self.final_activ.get_config()["activation"]})
        return config
