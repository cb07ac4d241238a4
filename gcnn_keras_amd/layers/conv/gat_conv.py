"""Attention heads of GAT / GATv2 (mirror of kgcnn/layers/conv/gat_conv.py:9-230) on the engine.

Both heads end in ``PoolingLocalEdgesAttention`` (segment softmax of the logits over each receiver's edges, then the
weighted segment sum - csrc/mp_segment.hip); they differ in how the logit is formed:

* GAT   (gat_conv.py:103-114): ``a_ij = act(a^T [W n_i || W n_j (|| e_ij)])``, messages ``W n_j``
* GATv2 (gat_conv.py:200-214): ``a_ij = a^T act(W_a [n_i || n_j (|| e_ij)])``, messages ``W n_j``

``call`` of every layer is that op sequence on the engine's layers (the *layer sequence*: every configuration, all
training - the attention pooling carries its reverse rules, ``autograd.SegmentSoftmax`` / ``WeightedSegmentSum``).

For the served sizes ``FusedAttentionBlock`` computes ``H`` heads over the same ``[nodes, edges, edge_index]`` with the
node-side Dense launches (GATv2: three per head; GAT: one per head plus one node-sized pass for all heads) and TWO
further launches whatever ``H`` is (csrc/mp_gat.hip, which states the algebra):
``mp_gat_logits_f32`` gathers two node rows per edge, adds the edge features' product and writes the logits ``(M, H)``,
the only edge-sized tensor; ``mp_gat_attend_f32`` runs the segment softmax and the weighted sum of the gathered messages
per (receiver, head) into ``(N, H, units)``.  The node-side products read row-block views of the layers' own kernels in
place (nothing is repacked: a copy could go stale under graph replay, see egnn_conv.py).  The per-edge dot product of the
layer sequence (``2F + D`` terms in one row) is summed here as two node-side products plus a ``D``-term one; the result
stays in the float32 class.

Served (``FUSED_ATTENTION_SIZES``, ``fused_attention_supported``): float32, ``units`` 32 or 64, at most 64 edge features
when ``use_edge_features`` (any width when not: the edges are not read), any node width, an activation among the engine's
codes, all heads of a block of one class with equal arguments, attention pooling at its defaults (``pooling_index`` 0,
``has_unconnected`` True).  Everything else, any call with keyword arguments and any call in grad mode where an input or
a weight requires grad takes the layer sequence, and so does ``use_fused_attention = False``.
"""
import ctypes

import torch

from ... import _ffi
from ..base import GraphBaseLayer
from ..gather import GatherNodesIngoing, GatherNodesOutgoing
from ..modules import Activation, Dense, LazyAverage, LazyConcatenate, _activation_name
from ..pooling import PoolingLocalEdgesAttention

_KERNEL_KEYS = ("kernel_regularizer", "activity_regularizer", "bias_regularizer", "kernel_constraint", "bias_constraint",
                "kernel_initializer", "bias_initializer")

FUSED_ATTENTION_SIZES = {"units": (32, 64), "max_edge_width": 64, "max_heads_per_launch": 8}   # csrc/mp_gat.hip


def fused_attention_supported(units, activation, use_edge_features=False, edge_width=None, dtype="float32",
                              pooling_index=0, has_unconnected=True, heads=None):
    """True when an attention block with these sizes runs on csrc/mp_gat.hip (the configuration decides).  ``edge_width``
    may be None while it is unknown and ``use_edge_features`` is off; ``heads``: the block's head layers, which must be
    of one class with equal arguments."""
    s = FUSED_ATTENTION_SIZES
    if dtype not in ("float32", torch.float32):
        return False
    if units not in s["units"]:
        return False
    if use_edge_features and (edge_width is None or not 0 <= int(edge_width) <= s["max_edge_width"]):
        return False
    if _activation_name(activation) not in _ffi.ACTIVATION_CODES:
        return False
    if pooling_index != 0 or not has_unconnected:
        return False
    if heads is not None:
        if len(heads) == 0 or any(type(h) is not type(heads[0]) for h in heads):
            return False
        first = _head_signature(heads[0])
        if any(_head_signature(h) != first for h in heads[1:]):
            return False
    return True


def _head_signature(head):
    pool = head.lay_pool_attention
    return (head.units, bool(head.use_edge_features), bool(head.use_final_activation), bool(head.use_bias),
            head._config_source().activation, pool.pooling_index, bool(pool.has_unconnected), bool(pool.is_sorted),
            head.dtype)


class FusedAttentionBlock:
    """``H`` attention heads of one class over the same inputs on csrc/mp_gat.hip.

    ``heads``: a list of ``AttentionHeadGAT`` or of ``AttentionHeadGATV2`` layers with equal arguments, or one
    ``MultiHeadGATV2Layer`` (whose per-head linear transform carries the activation).  ``block(nodes, edges, edge_index)``
    returns ``(stacked, logits)``: the heads' outputs as one values tensor ``(N, H, units)`` - ``stacked[:, k]`` is head
    ``k``, ``stacked.view(N, H * units)`` the concatenated heads - after the optional final activation, and the logits
    ``(M, H)`` in edge order.  More than 8 heads run in groups of 8 into the same two tensors.  No host read-back: the
    block can be captured into a HIP graph."""

    def __init__(self, heads):
        self.heads = [heads] if isinstance(heads, MultiHeadGATV2Layer) else list(heads)
        self.proto = self.heads[0]
        self.triples = [tri for h in self.heads for tri in h._dense_triples()]
        # the V2 form has a hidden logit Dense (AttentionHeadGATV2 and its subclass; AttentiveHeadFP without edge features)
        self.v2 = self.triples[0][1] is not None

    def supported(self, edge_width):
        """The configuration fits the kernels and every head's switch is on."""
        p = self.proto
        pool = p.lay_pool_attention
        return (all(h.use_fused_attention for h in self.heads)
                and fused_attention_supported(p.units, self.logit_activation(), p.use_edge_features, edge_width, p.dtype,
                                              pool.pooling_index, pool.has_unconnected,
                                              None if isinstance(p, MultiHeadGATV2Layer) else self.heads))

    def logit_activation(self):
        _, lay_aa, lay_a = self.triples[0]
        return (lay_aa if self.v2 else lay_a).activation

    def weight_tensors(self):
        return [t for tri in self.triples for lay in tri if lay is not None for t in (lay.kernel, lay.bias)
                if t is not None]

    def needs_grad(self, *inputs):
        """The kernels read the weights in place and have no reverse rule: any tape steps aside to the layer sequence."""
        from ...autograd import needs_grad
        return needs_grad(*inputs) or needs_grad(*self.weight_tensors())

    def route(self, nodes, edges, kwargs):
        """True when this call takes the fused kernels."""
        ev = edges.values
        width = int(ev.shape[-1]) if ev.dim() == 2 else None
        return (not kwargs and nodes.values.dtype == torch.float32 and nodes.values.dim() == 2
                and (not self.proto.use_edge_features or (ev.dtype == torch.float32 and ev.dim() == 2))
                and self.supported(width) and not self.needs_grad(nodes.values, ev))

    def __call__(self, nodes, edges, edge_index):
        from ..modules import dense_values
        p = self.proto
        hv = nodes.values
        _ffi.require_device(hv, edge_index.values)
        plan = edge_index.index_plan(nodes)
        plan.validate()
        n, e, u, f = plan.N, plan.M, p.units, int(hv.shape[1])
        if plan.K != 2 or n >= 2 ** 31 - 1 or e >= 2 ** 31 - 32:
            raise ValueError("the fused attention block takes (batch, [M], 2) indices of fewer than 2^31 nodes and edges")
        d, gv = 0, None
        if p.use_edge_features:
            gv = edges.values.detach().contiguous()
            _ffi.require_device(gv)
            d = int(gv.shape[1])
            if int(gv.shape[0]) != e:
                raise ValueError("the fused attention block: %d edge rows for %d edges" % (int(gv.shape[0]), e))
        hc = hv.detach().contiguous()
        code = _ffi.activation_code(self.logit_activation())
        ptr0, perm0, _ = plan.csr(0)
        num = len(self.triples)
        stacked = torch.empty((n, num, u), dtype=torch.float32, device=hv.device)
        logits = torch.empty((e, num), dtype=torch.float32, device=hv.device)
        group = FUSED_ATTENTION_SIZES["max_heads_per_launch"]
        for h0 in range(0, num, group):
            keep, ps, qs, wcs, bs, avs, wns = [], [], [], [], [], [], []   # `keep` holds the tensors until the launches
            for lay_lin, lay_aa, lay_a in self.triples[h0:h0 + group]:
                wn = dense_values(hc, lay_lin.kernel.detach(), None if lay_lin.bias is None else lay_lin.bias.detach(),
                                  lay_lin.activation)
                if self.v2:
                    # row blocks of the logit kernel, read in place (views: a repacked copy could go stale under replay)
                    wa = lay_aa.kernel.detach()
                    if int(wa.shape[0]) != 2 * f + d:
                        raise ValueError("the head was built for %d input columns, got %d" % (int(wa.shape[0]), 2 * f + d))
                    pp, qq = dense_values(hc, wa[:f], None, "linear"), dense_values(hc, wa[f:2 * f], None, "linear")
                    wc, bias, av = wa[2 * f:], None if lay_aa.bias is None else lay_aa.bias.detach(), lay_a.kernel.detach()
                else:
                    # p = Wn a[:U] and q = Wn a[U:2U] come from mp_gat_node_scores_f32 below, for all heads at once
                    av = lay_a.kernel.detach()
                    if int(av.shape[0]) != 2 * u + d:
                        raise ValueError("the head was built for %d input columns, got %d" % (int(av.shape[0]), 2 * u + d))
                    pp, qq, wc, bias = None, None, av[2 * u:], None
                keep += [wn, pp, qq, wc, bias, av]
                ps.append(None if pp is None else _ffi.ptr(pp).value)
                qs.append(None if qq is None else _ffi.ptr(qq).value)
                wcs.append(_ffi.ptr(wc).value if d > 0 else None)
                bs.append(None if bias is None else _ffi.ptr(bias).value)
                avs.append(None if av is None else _ffi.ptr(av).value)
                wns.append(_ffi.ptr(wn).value)
            k = len(ps)
            arr = lambda vals: (ctypes.c_void_p * k)(*vals)
            pq = None
            if not self.v2:
                pq = torch.empty((n, k, 4), dtype=torch.float32, device=hv.device)
                _ffi.call("mp_gat_node_scores_f32", k, u, arr(wns), arr(avs), n, _ffi.ptr(pq), _ffi.stream())
            _ffi.call("mp_gat_logits_f32", _ffi.MP_GAT_V2 if self.v2 else _ffi.MP_GAT_V1, k, u, arr(ps), arr(qs),
                      _ffi.ptr(pq), arr(wcs), arr(bs), arr(avs), n, _ffi.ptr(gv), d, _ffi.ptr(plan.cols), e,
                      _ffi.ptr(perm0), code, 0.05, _ffi.ptr(logits), num, h0, _ffi.stream())
            _ffi.call("mp_gat_attend_f32", k, u, arr(wns), n, _ffi.ptr(logits), num, h0, _ffi.ptr(plan.cols), e,
                      _ffi.ptr(ptr0), _ffi.ptr(perm0), _ffi.ptr(stacked), _ffi.stream())
            del keep
        if p.use_final_activation:
            stacked = p.lay_final_activ(nodes.with_values(stacked)).values
        return stacked, logits


class _AttentionHead(GraphBaseLayer):
    """Shared constructor surface and config of the two heads.  ``use_fused_attention`` (default True): sizes that fit
    ``fused_attention_supported`` run on the fused kernels outside a tape."""

    # no weight of the heads is left off the tape: Dense, the gathers, LazyConcatenate, Activation and the attention
    # pooling carry their rules
    weight_gradients = True

    def __init__(self, units, use_edge_features, use_final_activation, has_self_loops, activation, use_bias,
                 kernel_args, **kwargs):
        super().__init__(**kwargs)
        self.units = int(units)
        self.use_edge_features = use_edge_features
        self.use_final_activation = use_final_activation
        self.has_self_loops = has_self_loops
        self.use_bias = use_bias
        self._kernel_args = kernel_args
        self.lay_linear_trafo = Dense(units, activation="linear", use_bias=use_bias, **kernel_args)
        self._make_logit_layers(activation)
        self.lay_gather_in = GatherNodesIngoing()
        self.lay_gather_out = GatherNodesOutgoing()
        self.lay_concat = LazyConcatenate(axis=-1)
        self.lay_pool_attention = PoolingLocalEdgesAttention()
        if use_final_activation:
            self.lay_final_activ = Activation(activation=activation)
        self.use_fused_attention = True
        self._fused_block = None     # FusedAttentionBlock over this layer alone, made on the first call

    def build(self, input_shape):
        """``input_shape``: ``[nodes (batch, None, F), edges (batch, None, D), edge_index]``; creates every weight, in the
        order in which the layer sequence calls the Dense layers (the fused block reads the kernels directly)."""
        super().build(input_shape)
        f = int(input_shape[0][-1])
        d = int(input_shape[1][-1]) if self.use_edge_features else 0
        for lay_lin, lay_aa, lay_a in self._dense_triples():
            lay_lin.ensure_built((None, None, f))
            if lay_aa is not None:
                lay_aa.ensure_built((None, None, 2 * f + d))
                lay_a.ensure_built((None, None, self.units))
            else:
                lay_a.ensure_built((None, None, 2 * self.units + d))

    def _dense_triples(self):
        """Per head ``(message transform, hidden logit Dense or None, logit Dense)``."""
        return [(self.lay_linear_trafo, getattr(self, "lay_alpha_activation", None), self.lay_alpha)]

    def _own_block(self):
        if self._fused_block is None:
            self._fused_block = FusedAttentionBlock(self if isinstance(self, MultiHeadGATV2Layer) else [self])
        return self._fused_block

    def _call_fused(self, inputs, kwargs):
        """The head as a one-head block: its output, or None when the call takes the layer sequence."""
        node, edge, edge_index = inputs
        block = self._own_block()
        if not self.use_fused_attention or not block.route(node, edge, kwargs):
            return None
        stacked, _ = block(node, edge, edge_index)
        return node.with_values(stacked.view(stacked.shape[0], self.units))

    def _attend(self, node, messages, logits, edge_index, **kwargs):
        h = self.lay_pool_attention([node, messages, logits, edge_index], **kwargs)
        return self.lay_final_activ(h, **kwargs) if self.use_final_activation else h

    def _pair_features(self, left, right, edge, **kwargs):
        parts = [left, right, edge] if self.use_edge_features else [left, right]
        return self.lay_concat(parts, **kwargs)

    def get_config(self):
        config = super().get_config()
        config.update({"use_edge_features": self.use_edge_features, "use_bias": self.use_bias, "units": self.units,
                       "has_self_loops": self.has_self_loops, "use_final_activation": self.use_final_activation})
        sub = self._config_source().get_config()
        config.update({key: sub[key] for key in _KERNEL_KEYS + ("activation",)})
        return config


def _kernel_args(local_vars):
    return {key: local_vars[key] for key in _KERNEL_KEYS}


class AttentionHeadGAT(_AttentionHead):

    def __init__(self, units, use_edge_features=False, use_final_activation=True, has_self_loops=True,
                 activation="kgcnn>leaky_relu", use_bias=True, kernel_regularizer=None, bias_regularizer=None,
                 activity_regularizer=None, kernel_constraint=None, bias_constraint=None,
                 kernel_initializer="glorot_uniform", bias_initializer="zeros", **kwargs):
        super().__init__(units, use_edge_features, use_final_activation, has_self_loops, activation, use_bias,
                         _kernel_args(locals()), **kwargs)

    def _make_logit_layers(self, activation):
        self.lay_alpha = Dense(1, activation=activation, use_bias=False, **self._kernel_args)

    def _config_source(self):
        return self.lay_alpha

    def call(self, inputs, **kwargs):
        """inputs: ``[nodes (batch,[N],F), edges (batch,[M],Fe), edge_index (batch,[M],2)]`` -> ``(batch,[N],units)``."""
        fused = self._call_fused(inputs, kwargs)
        if fused is not None:
            return fused
        node, edge, edge_index = inputs
        w_n = self.lay_linear_trafo(node, **kwargs)
        wn_in = self.lay_gather_in([w_n, edge_index], **kwargs)
        wn_out = self.lay_gather_out([w_n, edge_index], **kwargs)
        logits = self.lay_alpha(self._pair_features(wn_in, wn_out, edge, **kwargs), **kwargs)   # (batch,[M],1)
        return self._attend(node, wn_out, logits, edge_index, **kwargs)


class AttentionHeadGATV2(_AttentionHead):

    def __init__(self, units, use_edge_features=False, use_final_activation=True, has_self_loops=True,
                 activation="kgcnn>leaky_relu", use_bias=True, kernel_regularizer=None, bias_regularizer=None,
                 activity_regularizer=None, kernel_constraint=None, bias_constraint=None,
                 kernel_initializer="glorot_uniform", bias_initializer="zeros", **kwargs):
        super().__init__(units, use_edge_features, use_final_activation, has_self_loops, activation, use_bias,
                         _kernel_args(locals()), **kwargs)

    def _make_logit_layers(self, activation):
        self.lay_alpha_activation = Dense(self.units, activation=activation, use_bias=self.use_bias, **self._kernel_args)
        self.lay_alpha = Dense(1, activation="linear", use_bias=False, **self._kernel_args)

    def _config_source(self):
        return self.lay_alpha_activation

    def call(self, inputs, **kwargs):
        """inputs: ``[nodes, edges, edge_index]`` as for ``AttentionHeadGAT``."""
        fused = self._call_fused(inputs, kwargs)
        if fused is not None:
            return fused
        node, edge, edge_index = inputs
        w_n = self.lay_linear_trafo(node, **kwargs)
        n_in = self.lay_gather_in([node, edge_index], **kwargs)
        n_out = self.lay_gather_out([node, edge_index], **kwargs)
        wn_out = self.lay_gather_out([w_n, edge_index], **kwargs)
        hidden = self.lay_alpha_activation(self._pair_features(n_in, n_out, edge, **kwargs), **kwargs)
        return self._attend(node, wn_out, self.lay_alpha(hidden, **kwargs), edge_index, **kwargs)


class MultiHeadGATV2Layer(AttentionHeadGATV2):
    r"""``num_heads`` GATv2 heads in one layer that also hands back the attention logits
    (kgcnn/layers/conv/gat_conv.py:233-323; MEGAN consumes the logits as edge importances).

    Returns ``(h, a)``: node embeddings ``(batch, [N], units * num_heads)`` (``concat_heads``) or their average
    ``(batch, [N], units)``, and the logits of all heads ``(batch, [M], num_heads, 1)``.  Like the reference, every head
    owns three Dense layers (``units`` with the activation, ``units`` with the activation, ``1`` linear) and reuses the
    base class's gathers, concatenation, attention pooling and optional final activation."""

    def __init__(self, units: int, num_heads: int, activation: str = "kgcnn>leaky_relu", use_bias: bool = True,
                 concat_heads: bool = True, **kwargs):
        super().__init__(units=units, activation=activation, use_bias=use_bias, **kwargs)
        self.num_heads = int(num_heads)
        self.concat_heads = concat_heads
        self.head_layers = []
        for _ in range(self.num_heads):
            self.head_layers += [Dense(units, activation=activation, use_bias=use_bias),
                                 Dense(units, activation=activation, use_bias=use_bias),
                                 Dense(1, activation="linear", use_bias=False)]
        self.lay_combine_heads = LazyConcatenate(axis=-1) if concat_heads else LazyAverage()

    def _dense_triples(self):
        return [tuple(self.head_layers[3 * k:3 * k + 3]) for k in range(self.num_heads)]

    def call(self, inputs, **kwargs):
        """inputs: ``[nodes, edges, edge_index]`` -> ``(node embeddings, attention logits)``."""
        node, edge, edge_index = inputs
        block = self._own_block()
        if self.use_fused_attention and block.route(node, edge, kwargs):
            stacked, logits = block(node, edge, edge_index)
            n, k, u = stacked.shape
            if self.concat_heads:
                h = node.with_values(stacked.view(n, k * u))
            else:
                h = self.lay_combine_heads([node.with_values(stacked[:, i]) for i in range(k)])
            return h, edge_index.with_values(logits.unsqueeze(-1))                               # (batch, [M], K, 1)
        n_in = self.lay_gather_in([node, edge_index], **kwargs)
        n_out = self.lay_gather_out([node, edge_index], **kwargs)
        pair = self._pair_features(n_in, n_out, edge, **kwargs)       # identical for every head
        logits, embeddings = [], []
        for k in range(self.num_heads):
            lay_linear, lay_alpha_activation, lay_alpha = self.head_layers[3 * k:3 * k + 3]
            wn_out = self.lay_gather_out([lay_linear(node, **kwargs), edge_index], **kwargs)
            a_ij = lay_alpha(lay_alpha_activation(pair, **kwargs), **kwargs)                     # (batch, [M], 1)
            embeddings.append(self._attend(node, wn_out, a_ij, edge_index, **kwargs))
            logits.append(a_ij)
        # the reference expands every head's logits to (batch, [M], 1, 1) and concatenates on axis -2; with a trailing
        # unit axis that is the last-axis concatenation of the (batch, [M], 1) logits, reshaped
        stacked = self.lay_concat(logits, **kwargs)
        stacked = stacked.with_values(stacked.values.unsqueeze(-1))                              # (batch, [M], K, 1)
        return self.lay_combine_heads(embeddings, **kwargs), stacked

    def get_config(self):
        config = super().get_config()
        config.update({"num_heads": self.num_heads, "concat_heads": self.concat_heads})
        return config
