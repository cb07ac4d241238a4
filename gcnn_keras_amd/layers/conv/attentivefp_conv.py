"""AttentiveFP layers (mirror of kgcnn/layers/conv/attentivefp_conv.py:9-236) on the engine.

``AttentiveHeadFP`` is a GATv2-shaped head whose context goes through ``activation_context``; with
``use_edge_features`` (the first layer of the model) both its message and its logit go through a per-edge non-linear
Dense on ``[n_j || e_ij]``.  ``PoolingNodesAttentive`` is the readout: a graph state, pooled from the nodes, is refined
``depth`` times by attention over the graph's nodes and a GRU cell.

``call`` of both layers is the reference's op sequence on the engine's layers (the *layer sequence*: every configuration,
all training - every op carries its reverse rule, the GRU cell through ``autograd.GRUCombine``).  Outside a tape the
served sizes take fused routes (csrc/mp_attentivefp.hip, which states the algebra):

* a head with edge features: three node-side Dense launches, ``mp_afp_edge_f32`` (per tile of 32 receiver-sorted
  positions the hidden row, the message and the logit; the message ``(M, units)`` is the only edge-sized feature tensor)
  and ``mp_afp_attend_f32`` (segment softmax, weighted sum and the context activation per receiver);
* a head without edge features is a GATv2 head with ``D = 0``: ``FusedAttentionBlock`` (layers/conv/gat_conv.py) on
  ``mp_gat_logits_f32`` / ``mp_gat_attend_f32`` plus one Activation call;
* the readout: one Dense launch and ``mp_afp_readout_f32``, the loop over ``depth`` inside the kernel.

The kernels read row-block views of the layers' own weights in place (nothing is repacked: a copy could go stale under
graph replay).  Served (``fused_attentive_head_supported`` / ``fused_attentive_readout_supported``): float32; heads:
``units`` 32 or 64, 1 to 64 edge features, a logit activation among ``_ffi.ACTIVATION_CODES``; readout: ``units`` a
multiple of 4 up to 256, sum or mean start pooling.  Everything else, any call with keyword arguments and any call in
grad mode where an input or a weight requires grad takes the layer sequence, and so does ``use_fused_attentive = False``.
"""
import torch

from ... import _ffi
from ...ops.segment import reduce_op_code
from ...ragged import RaggedTensor
from ..base import GraphBaseLayer, Layer
from ..gather import GatherNodesIngoing, GatherNodesOutgoing, GatherState
from ..modules import Activation, Dense, LazyConcatenate, _activation_name, dense_values
from ..pooling import PoolingLocalEdgesAttention, PoolingNodes, PoolingNodesAttention
from .gat_conv import FusedAttentionBlock
from .mpnn_conv import gru_cell_values

_KERNEL_KEYS = ("kernel_regularizer", "activity_regularizer", "bias_regularizer", "kernel_constraint", "bias_constraint",
                "kernel_initializer", "bias_initializer")

FUSED_ATTENTIVE_SIZES = {"head_units": (32, 64), "max_edge_width": 64,                  # csrc/mp_attentivefp.hip
                         "max_readout_units": _ffi.MP_AFP_READOUT_MAX_UNITS}


def fused_attentive_head_supported(units, activation, activation_context="elu", use_edge_features=False, edge_width=None,
                                   dtype="float32"):
    """True when a head with these sizes runs on the fused kernels (the configuration decides)."""
    s = FUSED_ATTENTIVE_SIZES
    if dtype not in ("float32", torch.float32) or units not in s["head_units"]:
        return False
    if _activation_name(activation) not in _ffi.ACTIVATION_CODES:
        return False
    if _activation_name(activation_context) not in _ffi.LAYER_ACTIVATION_CODES:
        return False
    if use_edge_features and (edge_width is None or not 1 <= int(edge_width) <= s["max_edge_width"]):
        return False
    return True


def fused_attentive_readout_supported(units, depth=3, pooling_method="sum", activation="kgcnn>leaky_relu",
                                      activation_context="elu", recurrent_activation="sigmoid", dtype="float32"):
    """True when a readout with these sizes runs on ``mp_afp_readout_f32`` (the configuration decides)."""
    if dtype not in ("float32", torch.float32):
        return False
    if units < 4 or units % 4 or units > FUSED_ATTENTIVE_SIZES["max_readout_units"] or int(depth) < 0:
        return False
    try:
        if reduce_op_code(pooling_method) not in (_ffi.MP_SUM, _ffi.MP_MEAN):
            return False
    except TypeError:
        return False
    return all(_activation_name(a) in _ffi.LAYER_ACTIVATION_CODES
               for a in (activation, activation_context, recurrent_activation))


def _needs_grad(layer, *values):
    from ...autograd import needs_grad
    return needs_grad(*values) or needs_grad(*[t for _, t in layer.weights])


class AttentiveHeadFP(GraphBaseLayer):
    r"""Attention head of AttentiveFP (attentivefp_conv.py:9-120): :math:`a_{ij} = a^T \sigma_1(W_a [h_i || h_j])`,
    :math:`\alpha_{ij} = \text{softmax}_j(a_{ij})`, :math:`C_i = \sigma_2(\sum_j \alpha_{ij} W h_j)`; with
    ``use_edge_features`` :math:`h_i \to \sigma_1(W_1 n_i)` and :math:`h_j \to \sigma_1(W_2 [n_j || e_{ij}])`.
    ``use_fused_attentive`` (default True): sizes that fit ``fused_attentive_head_supported`` run on the fused kernels
    outside a tape."""

    # no weight is left off the tape: Dense, the gathers, LazyConcatenate, Activation and the attention pooling carry
    # their rules
    weight_gradients = True
    use_final_activation = True   # FusedAttentionBlock's name for the context activation

    def __init__(self, units, use_edge_features=False, activation="kgcnn>leaky_relu", activation_context="elu",
                 use_bias=True, kernel_regularizer=None, bias_regularizer=None, activity_regularizer=None,
                 kernel_constraint=None, bias_constraint=None, kernel_initializer="glorot_uniform",
                 bias_initializer="zeros", **kwargs):
        super().__init__(**kwargs)
        self.use_edge_features = use_edge_features
        self.units = int(units)
        self.use_bias = use_bias
        local = locals()
        kernel_args = {key: local[key] for key in _KERNEL_KEYS}
        self.lay_linear_trafo = Dense(units, activation="linear", use_bias=use_bias, **kernel_args)
        self.lay_alpha_activation = Dense(units, activation=activation, use_bias=use_bias, **kernel_args)
        self.lay_alpha = Dense(1, activation="linear", use_bias=False, **kernel_args)
        self.lay_gather_in = GatherNodesIngoing()
        self.lay_gather_out = GatherNodesOutgoing()
        self.lay_concat = LazyConcatenate(axis=-1)
        self.lay_pool_attention = PoolingLocalEdgesAttention()
        self.lay_final_activ = Activation(activation=activation_context)
        if use_edge_features:
            self.lay_fc1 = Dense(units, activation=activation, use_bias=use_bias, **kernel_args)
            self.lay_fc2 = Dense(units, activation=activation, use_bias=use_bias, **kernel_args)
            self.lay_concat_edge = LazyConcatenate(axis=-1)
        self.use_fused_attentive = True
        self._fused_block = None     # FusedAttentionBlock over this layer alone (no edge features), made on first use

    # FusedAttentionBlock reads the switch under the GAT heads' name
    use_fused_attention = property(lambda self: self.use_fused_attentive)

    def build(self, input_shape):
        """``input_shape``: ``[nodes (batch, None, F), edges (batch, None, D), edge_index]``; creates every weight, in the
        order in which the layer sequence calls the Dense layers (the fused routes read the kernels directly)."""
        super().build(input_shape)
        f, u = int(input_shape[0][-1]), self.units
        if self.use_edge_features:
            d = int(input_shape[1][-1])
            self.lay_fc1.ensure_built((None, None, f))
            self.lay_fc2.ensure_built((None, None, f + d))
            f = u
        self.lay_linear_trafo.ensure_built((None, None, f))
        self.lay_alpha_activation.ensure_built((None, None, 2 * f))
        self.lay_alpha.ensure_built((None, None, u))

    def _dense_triples(self):
        return [(self.lay_linear_trafo, self.lay_alpha_activation, self.lay_alpha)]

    def _config_source(self):
        return self.lay_alpha_activation

    def fused_supported(self, edge_width):
        """The configuration fits the fused kernels (``edge_width`` is read with ``use_edge_features`` only)."""
        pool = self.lay_pool_attention
        return (pool.pooling_index == 0 and bool(pool.has_unconnected)
                and fused_attentive_head_supported(self.units, self.lay_alpha_activation.activation,
                                                   self.lay_final_activ.activation, self.use_edge_features, edge_width,
                                                   self.dtype))

    def _route_fused(self, node, edge, kwargs):
        """True when this call takes the fused kernels."""
        if kwargs or not self.use_fused_attentive:
            return False
        nv, ev = node.values, edge.values
        if nv.dtype != torch.float32 or nv.dim() != 2:
            return False
        if self.use_edge_features:
            if ev.dtype != torch.float32 or ev.dim() != 2 or not self.fused_supported(int(ev.shape[1])):
                return False
            return not _needs_grad(self, nv, ev)
        if self._fused_block is None:
            self._fused_block = FusedAttentionBlock([self])
        return self.fused_supported(None) and self._fused_block.route(node, edge, None)

    def _call_fused_edges(self, node, edge, edge_index):
        hv = node.values.detach().contiguous()
        gv = edge.values.detach().contiguous()
        _ffi.require_device(hv, gv, edge_index.values)
        plan = edge_index.index_plan(node)
        plan.validate()
        n, e, u, f, d = plan.N, plan.M, self.units, int(hv.shape[1]), int(gv.shape[1])
        if plan.K != 2 or n >= 2 ** 31 - 1 or e >= 2 ** 31 - 32:
            raise ValueError("the fused attentive head takes (batch, [M], 2) indices of fewer than 2^31 nodes and edges")
        if int(gv.shape[0]) != e:
            raise ValueError("the fused attentive head: %d edge rows for %d edges" % (int(gv.shape[0]), e))
        det = lambda t: None if t is None else t.detach()
        w2, wa, wl = det(self.lay_fc2.kernel), det(self.lay_alpha_activation.kernel), det(self.lay_linear_trafo.kernel)
        if tuple(w2.shape) != (f + d, u) or tuple(wa.shape) != (2 * u, u) or tuple(wl.shape) != (u, u):
            raise ValueError("the head was built for other input widths than (%d nodes, %d edges)" % (f, d))
        act = self.lay_alpha_activation.activation
        # row blocks of the layers' kernels, read in place (views: a repacked copy could go stale under replay)
        x = dense_values(hv, w2[:f], None, "linear")
        a1 = dense_values(hv, det(self.lay_fc1.kernel), det(self.lay_fc1.bias), self.lay_fc1.activation)
        p = dense_values(a1, wa[:u], None, "linear")
        ptr0, perm0, _ = plan.csr(0)
        logit = torch.empty((e,), dtype=torch.float32, device=hv.device)
        msg = torch.empty((e, u), dtype=torch.float32, device=hv.device)
        out = torch.empty((n, u), dtype=torch.float32, device=hv.device)
        _ffi.call("mp_afp_edge_f32", u, _ffi.ptr(x), _ffi.ptr(p), n, _ffi.ptr(gv), d, _ffi.ptr(w2[f:]),
                  _ffi.ptr(det(self.lay_fc2.bias)), _ffi.ptr(wl), _ffi.ptr(det(self.lay_linear_trafo.bias)),
                  _ffi.ptr(wa[u:]), _ffi.ptr(det(self.lay_alpha_activation.bias)), _ffi.ptr(det(self.lay_alpha.kernel)),
                  _ffi.ptr(plan.cols), e, _ffi.ptr(perm0), _ffi.activation_code(act), 0.05, _ffi.ptr(logit),
                  _ffi.ptr(msg), _ffi.stream())
        _ffi.call("mp_afp_attend_f32", u, _ffi.ptr(msg), _ffi.ptr(logit), n, _ffi.ptr(plan.cols), e, _ffi.ptr(ptr0),
                  _ffi.ptr(perm0), _ffi.activation_code(self.lay_final_activ.activation), 0.05, _ffi.ptr(out),
                  _ffi.stream())
        return node.with_values(out)

    def call(self, inputs, **kwargs):
        """inputs: ``[nodes (batch,[N],F), edges (batch,[M],D), edge_index (batch,[M],2)]`` -> ``(batch,[N],units)``."""
        node, edge, edge_index = inputs
        if self._route_fused(node, edge, kwargs):
            if self.use_edge_features:
                return self._call_fused_edges(node, edge, edge_index)
            stacked, _ = self._fused_block(node, edge, edge_index)
            return node.with_values(stacked.view(stacked.shape[0], self.units))
        n_in = self.lay_gather_in([node, edge_index], **kwargs)
        n_out = self.lay_gather_out([node, edge_index], **kwargs)
        if self.use_edge_features:
            n_in = self.lay_fc1(n_in, **kwargs)
            n_out = self.lay_concat_edge([n_out, edge], **kwargs)
            n_out = self.lay_fc2(n_out, **kwargs)
        wn_out = self.lay_linear_trafo(n_out, **kwargs)
        e_ij = self.lay_concat([n_in, n_out], **kwargs)
        e_ij = self.lay_alpha_activation(e_ij, **kwargs)
        a_ij = self.lay_alpha(e_ij, **kwargs)                                                    # (batch, [M], 1)
        n_i = self.lay_pool_attention([node, wn_out, a_ij, edge_index], **kwargs)
        return self.lay_final_activ(n_i, **kwargs)

    def get_config(self):
        config = super().get_config()
        config.update({"use_edge_features": self.use_edge_features, "use_bias": self.use_bias, "units": self.units})
        sub = self.lay_alpha_activation.get_config()
        config.update({key: sub[key] for key in _KERNEL_KEYS + ("activation",)})
        config.update({"activation_context": self.lay_final_activ.get_config()["activation"]})
        return config


class _GRUCell(Layer):
    """The weights of ``ks.layers.GRUCell(units)`` in the Keras layout that ``GRUUpdate`` holds (``reset_after=True``):
    ``kernel (in, 3u)``, ``recurrent_kernel (u, 3u)``, ``bias (2, 3u)``, gates ``[z | r | h]``; ``call([x, h])`` is one
    step, on the tape when an operand needs grad."""

    weight_gradients = True

    def __init__(self, units, conf):
        super().__init__(name="gru_cell")
        self.units, self._conf = int(units), conf
        self.act = _ffi.activation_code("tanh")
        self.rec_act = _ffi.activation_code(conf["recurrent_activation"])
        self.kernel = self.recurrent_kernel = self.bias = None

    def build(self, input_shape):
        super().build(input_shape)
        u = self.units
        self.kernel = self.add_weight("kernel", (int(input_shape[-1]), 3 * u), self._conf["kernel_initializer"])
        self.recurrent_kernel = self.add_weight("recurrent_kernel", (u, 3 * u), self._conf["recurrent_initializer"])
        if self._conf["use_bias"]:
            self.bias = self.add_weight("bias", (2, 3 * u), self._conf["bias_initializer"])

    def call(self, inputs, **kwargs):
        x, h = inputs
        return gru_cell_values(x, h, self.kernel, self.recurrent_kernel, self.bias, self.act, self.rec_act)


class PoolingNodesAttentive(GraphBaseLayer):
    r"""Attentive readout of AttentiveFP (attentivefp_conv.py:123-236): the pooled nodes are the start state ``h`` of a
    GRU cell; ``depth`` times ``a_i = \sigma_1(w^T [h || n_i])``, ``c = \sigma_2(\sum_i softmax_i(a_i) W n_i)``,
    ``h = GRUCell(c, h)``.  Returns ``(batch, units)`` with ``PoolingNodes``' row count: trailing empty graphs are
    dropped, interior ones run the recurrence on ``c = \sigma_2(0)``.  ``use_fused_attentive`` (default True): sizes that
    fit ``fused_attentive_readout_supported`` run on ``mp_afp_readout_f32`` outside a tape."""

    weight_gradients = True   # Dense, GatherState, the attention pooling and the GRU cell carry their rules

    def __init__(self, units, depth=3, pooling_method="sum", activation="kgcnn>leaky_relu", activation_context="elu",
                 use_bias=True, kernel_regularizer=None, bias_regularizer=None, activity_regularizer=None,
                 kernel_constraint=None, bias_constraint=None, kernel_initializer="glorot_uniform",
                 bias_initializer="zeros", recurrent_activation="sigmoid", recurrent_initializer="orthogonal",
                 recurrent_regularizer=None, recurrent_constraint=None, dropout=0.0, recurrent_dropout=0.0,
                 reset_after=True, **kwargs):
        super().__init__(**kwargs)
        if not reset_after or dropout or recurrent_dropout:
            raise NotImplementedError("PoolingNodesAttentive is built for the Keras default cell: reset_after=True, no "
                                      "dropout")
        self.pooling_method = pooling_method
        self.depth = int(depth)
        self.units = int(units)
        local = locals()
        kernel_args = {key: local[key] for key in ("use_bias",) + _KERNEL_KEYS}
        self._gru_conf = {"recurrent_activation": recurrent_activation, "use_bias": use_bias,
                          "kernel_initializer": kernel_initializer, "recurrent_initializer": recurrent_initializer,
                          "bias_initializer": bias_initializer, "recurrent_regularizer": recurrent_regularizer,
                          "recurrent_constraint": recurrent_constraint, "dropout": dropout,
                          "recurrent_dropout": recurrent_dropout, "reset_after": reset_after}
        self.lay_linear_trafo = Dense(units, activation="linear", **kernel_args)
        self.lay_alpha = Dense(1, activation=activation, **kernel_args)
        self.lay_gather_s = GatherState()
        self.lay_concat = LazyConcatenate(axis=-1)
        self.lay_pool_start = PoolingNodes(pooling_method=self.pooling_method)
        self.lay_pool_attention = PoolingNodesAttention()
        self.lay_final_activ = Activation(activation=activation_context)
        self.lay_gru = _GRUCell(units, self._gru_conf)
        self.use_fused_attentive = True

    def build(self, input_shape):
        """``input_shape``: nodes ``(batch, None, units)``; creates every weight in the order of the layer sequence."""
        super().build(input_shape)
        f = int(input_shape[-1])
        if f != self.units:
            raise ValueError("PoolingNodesAttentive: the pooled nodes are the GRU state, so the node width (%d) must equal "
                             "units (%d)" % (f, self.units))
        self.lay_linear_trafo.ensure_built((None, None, f))
        self.lay_alpha.ensure_built((None, None, 2 * f))
        self.lay_gru.ensure_built((None, self.units))

    def fused_supported(self):
        return fused_attentive_readout_supported(self.units, self.depth, self.pooling_method, self.lay_alpha.activation,
                                                 self.lay_final_activ.activation, self._gru_conf["recurrent_activation"],
                                                 self.dtype)

    @staticmethod
    def _without_trailing_empty(node):
        """``node`` cut to the graphs ``PoolingNodes`` returns a row for (its trailing empty graphs dropped)."""
        splits = node.row_splits_host()
        rows = g = node.nrows()
        while rows > 0 and splits[rows] == splits[rows - 1]:
            rows -= 1
        if rows == g:
            return node
        out = RaggedTensor(node.values, node.row_splits[:rows + 1])
        out._splits_host = splits[:rows + 1]
        return out

    def _call_fused(self, node):
        vals = node.values.detach().contiguous()
        _ffi.require_device(vals, node.row_splits)
        n, g, u = int(vals.shape[0]), node.nrows(), self.units
        det = lambda t: None if t is None else t.detach()
        lin, gru = self.lay_linear_trafo, self.lay_gru
        wn = dense_values(vals, det(lin.kernel), det(lin.bias), "linear") if (n > 0 and self.depth > 0) else None
        b_in = det(gru.bias)[0] if gru.bias is not None else None
        b_rec = det(gru.bias)[1] if gru.bias is not None else None
        out = torch.empty((g, u), dtype=torch.float32, device=vals.device)
        term = torch.empty((max(n, 1),), dtype=torch.float64, device=vals.device)   # the kernel's node-sized workspace
        _ffi.call("mp_afp_readout_f32", _ffi.ptr(vals), _ffi.ptr(wn), n, _ffi.ptr(node.row_splits), g, u, self.depth,
                  reduce_op_code(self.pooling_method), _ffi.ptr(det(self.lay_alpha.kernel)),
                  _ffi.ptr(det(self.lay_alpha.bias)), _ffi.ptr(det(gru.kernel)), _ffi.ptr(det(gru.recurrent_kernel)),
                  _ffi.ptr(b_in), _ffi.ptr(b_rec), _ffi.activation_code(self.lay_alpha.activation), 0.05,
                  _ffi.activation_code(self.lay_final_activ.activation), gru.act, gru.rec_act, _ffi.ptr(term),
                  _ffi.ptr(out), _ffi.stream())
        return out

    def call(self, inputs, **kwargs):
        """inputs: nodes ``(batch, [N], units)`` -> ``(batch, units)``."""
        node = self._without_trailing_empty(self.assert_ragged_input_rank(inputs))
        if (not kwargs and self.use_fused_attentive and node.values.dtype == torch.float32 and node.values.dim() == 2
                and self.fused_supported() and not _needs_grad(self, node.values)):
            return self._call_fused(node)
        h = self.lay_pool_start(node, **kwargs)
        wn = self.lay_linear_trafo(node, **kwargs)
        for _ in range(self.depth):
            hv = self.lay_gather_s([h, node], **kwargs)
            ev = self.lay_concat([hv, node], **kwargs)
            av = self.lay_alpha(ev, **kwargs)
            cont = self.lay_pool_attention([wn, av], **kwargs)
            cont = self.lay_final_activ(cont, **kwargs)
            h = self.lay_gru([cont, h], **kwargs)
        return h

    def get_config(self):
        config = super().get_config()
        config.update({"units": self.units, "depth": self.depth, "pooling_method": self.pooling_method})
        sub = self.lay_alpha.get_config()
        config.update({key: sub[key] for key in _KERNEL_KEYS + ("activation", "use_bias")})
        config.update({"activation_context": self.lay_final_activ.get_config()["activation"]})
        config.update({key: self._gru_conf[key] for key in ("recurrent_activation", "recurrent_initializer",
                                                            "recurrent_regularizer", "recurrent_constraint", "dropout",
                                                            "recurrent_dropout", "reset_after")})
        return config
