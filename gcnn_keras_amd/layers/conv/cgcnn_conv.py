"""``CGCNNLayer`` (mirror of kgcnn/layers/conv/cgcnn_conv.py:9-128) and its fused gate step on csrc/mp_cgcnn.hip.

The reference gathers both end nodes of every edge, concatenates ``[h_i, h_j, g]`` into an ``(M, 2F + D)`` tensor, runs
the two Dense layers ``s`` and ``f`` on it, optionally batch-normalises both, multiplies ``act_s(.) * sigmoid(.)``, sums
into the receivers and updates ``h' = act_out(h + BN_out(u))``.  ``message_function`` / ``update_nodes`` are that op
sequence on the engine's layers (the *layer sequence*: every configuration, all training).

For the default sizes ``FusedGateStep`` computes the same layer in five launches: the four node-side products ``h Wa_s``,
``h Wa_f``, ``h Wb_s``, ``h Wb_f`` (``mp_dense_f32`` on row-block views of the two kernels, read in place) and
``mp_cgcnn_gate_f32``, which gathers one row of each per edge, adds the edge features' product (matrix pipe) and the
bias, applies the batch-norm affines, the activations and the gate, sums per receiver in edge order and finishes with the
node update.  None of the edge-sized intermediates is written.  The per-edge dot product of the layer sequence (``2F +
D`` terms in one row) is summed here as two node-side 64-term products plus a ``D``-term one; the result stays in the
float32 class.

Served sizes (``FUSED_GATE_SIZES``, ``fused_gate_supported``): node width = units = 64, ``1 <= D <= 64`` edge features,
``use_bias`` either way, ``activation_s`` / ``activation_out`` among the engine's codes, batch normalisation on or off
(inference mode, last axis), sum pooling into index column 0, float32.  The fused step is forward-only: a call in grad
mode where an input or a weight requires grad takes the layer sequence, and so does ``layer.use_fused_gate = False``.
Edge lists that are not receiver-sorted are served through the plan's CSR permutation.
"""
import ctypes

import torch

from ... import _ffi
from ..message import MessagePassingBase
from ..modules import Activation, Dense, LazyAdd, LazyConcatenate, LazyMultiply, _activation_name
from ..norm import GraphBatchNormalization

FUSED_GATE_SIZES = {"units": 64, "max_edge_width": 64}   # csrc/mp_cgcnn.hip


def fused_gate_supported(node_width, units, edge_width, activation_s, activation_out, pooling_method,
                         pooling_index=0, dtype="float32"):
    """True when one ``CGCNNLayer`` with these sizes runs on ``mp_cgcnn_gate_f32`` (the configuration decides)."""
    s = FUSED_GATE_SIZES
    if node_width != s["units"] or units != s["units"]:
        return False
    if edge_width is None or not 1 <= int(edge_width) <= s["max_edge_width"]:
        return False
    if any(_activation_name(act) not in _ffi.ACTIVATION_CODES for act in (activation_s, activation_out)):
        return False
    if dtype not in ("float32", torch.float32):
        return False
    return pooling_method in ("sum", "segment_sum", "reduce_sum") and pooling_index == 0


class FusedGateStep:
    """One ``CGCNNLayer`` on ``mp_cgcnn_gate_f32``: ``step(h, edges, edge_index)`` returns the updated nodes."""

    def __init__(self, layer):
        self.layer = layer

    def weight_tensors(self):
        return [t for _, t in self.layer.weights if t is not None]

    def needs_grad(self, *inputs):
        """The kernel reads the weights in place and has no reverse rule: any tape steps aside to the layer sequence."""
        from ...autograd import needs_grad
        return needs_grad(*inputs) or needs_grad(*self.weight_tensors())

    def __call__(self, h, edges, edge_index):
        from ..modules import dense_values
        lay = self.layer
        hv, gv = h.values, edges.values
        _ffi.require_device(hv, gv, edge_index.values)
        f = FUSED_GATE_SIZES["units"]
        if hv.dtype != torch.float32 or gv.dtype != torch.float32 or hv.dim() != 2 or gv.dim() != 2:
            raise ValueError("the fused CGCNN gate step expects float32 nodes (batch, [N], 64) and edges (batch, [M], D)")
        d = int(gv.shape[1])
        plan = edge_index.index_plan(h)
        plan.validate()
        n, e = plan.N, plan.M
        if plan.K != 2 or e != int(gv.shape[0]) or int(hv.shape[1]) != f:
            raise ValueError("the fused CGCNN gate step: %d edge rows for %d edges of %d columns, node width %d"
                             % (int(gv.shape[0]), e, plan.K, int(hv.shape[1])))
        if n >= 2 ** 31 - 1 or e >= 2 ** 31 - 32:
            raise ValueError("the fused CGCNN gate step indexes nodes and edges with 32 bits")
        # row blocks of the two Dense kernels, read in place (views: a repacked copy could go stale under graph replay)
        ks, kf = lay.s.kernel.detach(), lay.f.kernel.detach()
        if tuple(ks.shape) != (2 * f + d, f):
            raise ValueError("the layer was built for %d edge features, got %d" % (int(ks.shape[0]) - 2 * f, d))
        hc = hv.detach().contiguous()
        pa_s, pa_f = dense_values(hc, ks[:f], None, "linear"), dense_values(hc, kf[:f], None, "linear")
        pb_s, pb_f = dense_values(hc, ks[f:2 * f], None, "linear"), dense_values(hc, kf[f:2 * f], None, "linear")
        bn = eps = None
        if lay.batch_normalization:
            norms = (lay.batch_norm_s, lay.batch_norm_f, lay.batch_norm_out)
            ptrs = []
            for b in norms:
                ptrs += [_ffi.ptr(b.gamma), _ffi.ptr(b.beta), _ffi.ptr(b.moving_mean), _ffi.ptr(b.moving_variance)]
            bn = (ctypes.c_void_p * 12)(*ptrs)
            eps = (ctypes.c_float * 3)(*[b.epsilon for b in norms])
        ptr0, perm0, _ = plan.csr(0)
        ws, nbytes = _ffi.float_workspace("mp_cgcnn_gate_ws_bytes", e, device=hv.device)
        out = torch.empty((n, f), dtype=torch.float32, device=hv.device)
        bias_s = None if lay.s.bias is None else lay.s.bias.detach()
        bias_f = None if lay.f.bias is None else lay.f.bias.detach()
        _ffi.call("mp_cgcnn_gate_f32", _ffi.ptr(hc), _ffi.ptr(pa_s), _ffi.ptr(pa_f), _ffi.ptr(pb_s), _ffi.ptr(pb_f), n,
                  _ffi.ptr(gv.detach().contiguous()), d, _ffi.ptr(plan.cols), e, _ffi.ptr(ptr0), _ffi.ptr(perm0),
                  _ffi.ptr(ks[2 * f:]), _ffi.ptr(kf[2 * f:]), _ffi.ptr(bias_s), _ffi.ptr(bias_f), bn, eps,
                  _ffi.activation_code(lay.activation_s_layer.activation),
                  _ffi.activation_code(lay.activation_out_layer.activation), 0.05, _ffi.ptr(ws), nbytes, _ffi.ptr(out),
                  _ffi.stream())
        return h.with_values(out)


class CGCNNLayer(MessagePassingBase):
    r"""Message passing layer of the Crystal Graph Convolutional Neural Network
    (`CGCNN <https://journals.aps.org/prl/abstract/10.1103/PhysRevLett.120.145301>`_; kgcnn/layers/conv/cgcnn_conv.py:9-128).

    ``layer([nodes (batch, [N], F), edges (batch, [M], D), edge_index (batch, [M], 2)])`` returns the updated nodes.
    Sublayers (and so the weights) come in the reference's order: ``batch_norm_f``, ``batch_norm_s``, ``batch_norm_out``
    (each ``gamma, beta, moving_mean, moving_variance``), then ``f``, ``s`` (each ``kernel, bias``).
    ``use_fused_gate`` (default True): sizes that fit ``fused_gate_supported`` run on the fused kernel outside a tape."""

    # no weight of this layer is left off the tape: Dense, Activation, Lazy* and the pooling carry their rules; a
    # GraphBatchNormalization sublayer has no weight gradients and raises by itself in grad mode (layers/base.py)
    weight_gradients = True

    def __init__(self, units: int = 64, activation_s="softplus", activation_out="softplus",
                 batch_normalization: bool = False, use_bias: bool = True, kernel_regularizer=None,
                 bias_regularizer=None, activity_regularizer=None, kernel_constraint=None, bias_constraint=None,
                 kernel_initializer="glorot_uniform", bias_initializer="zeros", **kwargs):
        super().__init__(**kwargs)
        self.units = units
        self.use_bias = use_bias
        self.batch_normalization = batch_normalization
        kernel_args = {"kernel_regularizer": kernel_regularizer, "bias_regularizer": bias_regularizer,
                       "kernel_constraint": kernel_constraint, "bias_constraint": bias_constraint,
                       "kernel_initializer": kernel_initializer, "bias_initializer": bias_initializer}
        self.activation_f_layer = Activation(activation="sigmoid", activity_regularizer=activity_regularizer)
        self.activation_s_layer = Activation(activation_s, activity_regularizer=activity_regularizer)
        self.activation_out_layer = Activation(activation_out, activity_regularizer=activity_regularizer)
        if batch_normalization:
            self.batch_norm_f = GraphBatchNormalization()
            self.batch_norm_s = GraphBatchNormalization()
            self.batch_norm_out = GraphBatchNormalization()
        self.f = Dense(self.units, activation="linear", use_bias=use_bias, **kernel_args)
        self.s = Dense(self.units, activation="linear", use_bias=use_bias, **kernel_args)
        self.lazy_mult = LazyMultiply()
        self.lazy_add = LazyAdd()
        self.lazy_concat = LazyConcatenate(axis=2)
        self.use_fused_gate = True
        self._fused_step = FusedGateStep(self)
        self.fused_gate = None      # decided in build(): the sizes fit the fused kernel

    def build(self, input_shape):
        """``input_shape``: ``[nodes (batch, None, F), edges (batch, None, D), edge_index]``; creates every weight."""
        super().build(input_shape)
        node_width, edge_width = int(input_shape[0][-1]), int(input_shape[1][-1])
        width = 2 * node_width + edge_width
        if self.batch_normalization:
            self.batch_norm_f.ensure_built((None, None, self.units))
            self.batch_norm_s.ensure_built((None, None, self.units))
            self.batch_norm_out.ensure_built((None, None, self.units))
        self.f.ensure_built((None, None, width))
        self.s.ensure_built((None, None, width))
        self.fused_gate = fused_gate_supported(node_width, self.units, edge_width, self.activation_s_layer.activation,
                                               self.activation_out_layer.activation, self.pooling_method,
                                               self.lay_pool_default.pooling_index, self.dtype)

    def message_function(self, inputs, **kwargs):
        r"""inputs: ``[nodes_in, nodes_out, edges]`` -> gated messages ``(batch, [M], units)``."""
        nodes_in, nodes_out, edge_features = inputs
        x = self.lazy_concat([nodes_in, nodes_out, edge_features], **kwargs)
        x_s, x_f = self.s(x, **kwargs), self.f(x, **kwargs)
        if self.batch_normalization:
            x_s, x_f = self.batch_norm_s(x_s, **kwargs), self.batch_norm_f(x_f, **kwargs)
        x_s, x_f = self.activation_s_layer(x_s, **kwargs), self.activation_f_layer(x_f, **kwargs)
        return self.lazy_mult([x_s, x_f], **kwargs)

    def update_nodes(self, inputs, **kwargs):
        r"""inputs: ``[nodes, node_updates]`` -> ``act_out(nodes + BN_out(node_updates))``."""
        nodes, nodes_update = inputs
        if self.batch_normalization:
            nodes_update = self.batch_norm_out(nodes_update, **kwargs)
        nodes_updated = self.lazy_add([nodes, nodes_update], **kwargs)
        return self.activation_out_layer(nodes_updated, **kwargs)

    def call(self, inputs, **kwargs):
        nodes, edges, edge_index = inputs
        if (self.fused_gate and self.use_fused_gate and not kwargs
                and not self._fused_step.needs_grad(nodes.values, edges.values)):
            return self._fused_step(nodes, edges, edge_index)
        return super().call(inputs, **kwargs)

    def get_config(self):
        """The reference's keys (cgcnn_conv.py:113-128): the Dense arguments are read back from ``f``."""
        config = super().get_config()
        dense = self.f.get_config()
        config.update({"units": self.units, "use_bias": self.use_bias, "batch_normalization": self.batch_normalization,
                       "activation_s": self.activation_s_layer.activation,
                       "activation_out": self.activation_out_layer.activation,
                       "activity_regularizer": self.activation_out_layer.activity_regularizer})
        config.update({key: dense[key] for key in ("kernel_regularizer", "bias_regularizer", "kernel_constraint",
                                                   "bias_constraint", "kernel_initializer", "bias_initializer")})
        return config
