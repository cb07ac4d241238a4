"""The edge step of one INorp block (this engine's own layer; the reference spells it inline,
kgcnn/literature/INorp.py:119-127).

``INorpEdgeStep([nodes, edges, edge_index])`` returns, per node, the pooled output of the block's edge MLP on
``[n[outgoing] || n[ingoing] || edges]``.  It is built around the block's ``GraphMLP`` and ``PoolingLocalEdges`` and owns no
weight of its own.  It has two routes:

* the *layer sequence*, the reference's ops (``GatherNodesIngoing``, ``GatherNodesOutgoing``, two ``LazyConcatenate``,
  ``GraphMLP``, ``PoolingLocalEdges``): the default, every configuration, every call with keyword arguments;
* the *fused route* (``use_fused_step = True``) for an edge MLP ``Dense(H1, act) -> Dense(H2, linear)``.  The last layer
  is linear, so it commutes with the pool, and the first is linear in its three column blocks:

      nu[r] = (pool_e act(Pj[send e] + Pi[recv e] + edges[e] Wc)) W2 + c[r] b2

  with ``Pj = n W1[0:F]``, ``Pi = n W1[F:2F] + b1``, ``Wc = W1[2F:2F+Fe]`` (row-block views of the first kernel, read in
  place; the outgoing node, index column 1, owns the first block) and ``c`` the receiver's edge count for a sum,
  ``[count > 0]`` for a mean.  Two node-sized Dense launches, ``mp_inorp_edge_f32`` (csrc/mp_inorp.hip) and one more Dense
  on the nodes; no edge-sized tensor is written.  On a tape (an input or a weight of the step requires grad) the kernel
  runs inside ``autograd.InorpEdge``, whose backward recomputes the pre-activation; the Dense launches stay ``Dense`` rules,
  so torch's accumulation assembles the gradients of the four weights and of the nodes.

Served sizes (``fused_step_supported``, decided in ``build``): float32; exactly two Dense layers without normalisation or
dropout, the second linear, both with or both without bias; the first activation among the engine's codes; ``H1`` in
{16, 32, 64, 128}; ``H2`` a multiple of 4 up to 128; edge width 1 to 64; any node width; sum or mean pooling on index 0.
"""
import torch

from ... import _ffi
from ..base import GraphBaseLayer
from ..gather import GatherNodesIngoing, GatherNodesOutgoing
from ..mlp import GraphMLP
from ..modules import LazyConcatenate, _activation_name, binary_values, dense_values
from ..pooling import PoolingLocalEdges

FUSED_STEP_SIZES = {"hidden": (16, 32, 64, 128), "max_units": 128, "max_edge_width": 64}   # csrc/mp_inorp.hip
_FUSED_POOLING = {"mean": _ffi.MP_MEAN, "segment_mean": _ffi.MP_MEAN, "reduce_mean": _ffi.MP_MEAN,
                  "sum": _ffi.MP_SUM, "segment_sum": _ffi.MP_SUM, "reduce_sum": _ffi.MP_SUM}


def fused_step_supported(node_width, edge_width, units, activation, use_bias, pooling_method, pooling_index=0,
                         dtype="float32", plain=True):
    """True when the edge step with these sizes runs on the fused route (the configuration decides).  ``units``,
    ``activation`` and ``use_bias`` are the edge MLP's per-layer lists; ``plain`` is false when one of its layers uses
    normalisation or dropout."""
    s = FUSED_STEP_SIZES
    if node_width is None or edge_width is None or not plain:
        return False
    if dtype not in ("float32", torch.float32):
        return False
    units, activation, use_bias = list(units), list(activation), list(use_bias)
    if len(units) != 2 or len(activation) != 2 or len(use_bias) != 2:
        return False
    if _activation_name(activation[1]) != "linear" or _activation_name(activation[0]) not in _ffi.ACTIVATION_CODES:
        return False
    if bool(use_bias[0]) != bool(use_bias[1]):
        return False
    h1, h2 = int(units[0]), int(units[1])
    if h1 not in s["hidden"] or h2 < 4 or h2 % 4 or h2 > s["max_units"]:
        return False
    if int(node_width) < 1 or not 1 <= int(edge_width) <= s["max_edge_width"]:
        return False
    return pooling_method in _FUSED_POOLING and pooling_index == 0


class EdgeStepSpec:
    """The index side, activation and pooling of one fused step, for ``autograd.InorpEdge``: ``forward`` is the launch
    of ``mp_inorp_edge_f32`` on values tensors, ``grad`` its reverse."""

    def __init__(self, nodes, edges, edge_index, activation, pooling_method):
        self.plan = edge_index.index_plan(nodes)
        self.plan.validate()
        ev = edges.values
        _ffi.require_device(nodes.values, ev)
        if ev.dtype != torch.float32 or ev.dim() != 2 or int(ev.shape[0]) != self.plan.M or self.plan.K != 2:
            raise ValueError("the fused INorp step expects float32 edges (batch, [M], Fe) over an edge index of two "
                             "columns, got %s for %d edges of %d columns" % (tuple(ev.shape), self.plan.M, self.plan.K))
        self.n, self.e, self.fe = self.plan.N, self.plan.M, int(ev.shape[1])
        self.act = _ffi.activation_code(_activation_name(activation))
        self.op = _FUSED_POOLING[pooling_method]

    def _args(self, pj, pi, ev, wc):
        ptr0, perm0, _ = self.plan.csr(0)
        h1 = int(pj.shape[1])
        ws, nbytes = _ffi.float_workspace("mp_inorp_edge_ws_bytes", self.e, h1, device=pj.device)
        head = [_ffi.ptr(pj), _ffi.ptr(pi), self.n, h1, _ffi.ptr(ev), self.fe, _ffi.ptr(wc), _ffi.ptr(self.plan.cols),
                self.e, _ffi.ptr(ptr0), _ffi.ptr(perm0), self.act, 0.05, self.op]
        return head, ws, nbytes, h1

    def forward(self, pj, pi, ev, wc):
        """``out (N, H1)`` of the contiguous values ``pj``, ``pi`` (N, H1), ``ev`` (E, Fe) and ``wc`` (Fe, H1)."""
        head, ws, nbytes, h1 = self._args(pj, pi, ev, wc)
        out = torch.empty((self.n, h1), dtype=torch.float32, device=pj.device)
        _ffi.call("mp_inorp_edge_f32", *head, _ffi.ptr(ws), nbytes, _ffi.ptr(out), _ffi.stream())
        return out

    def grad(self, pj, pi, ev, wc, g, want_pj=True, want_edges=False, want_wc=True):
        """``(Pj_bar, Pi_bar, edges_bar, Wc_bar)`` of the upstream gradient ``g`` (N, H1) of ``out``."""
        from ...autograd import dense_wgrad
        from ...ops.segment import _segment_reduce_raw
        from ..modules import _dense_raw
        head, ws, nbytes, h1 = self._args(pj, pi, ev, wc)
        dev = g.device
        gz = torch.empty((self.e, h1), dtype=torch.float32, device=dev)
        pi_bar = torch.empty((self.n, h1), dtype=torch.float32, device=dev)
        _ffi.call("mp_inorp_edge_grad_f32", *head, _ffi.ptr(g), _ffi.ptr(ws), nbytes, _ffi.ptr(gz), _ffi.ptr(pi_bar),
                  _ffi.stream())
        if self.e == 0:   # nothing reaches the senders, the edge block of the kernel or the edges
            return (torch.zeros_like(pi_bar) if want_pj else None, pi_bar,
                    torch.zeros_like(ev) if want_edges else None, torch.zeros_like(wc) if want_wc else None)
        pj_bar = wc_bar = e_bar = None
        if want_pj:
            ptr1, perm1, _ = self.plan.csr(1)
            pj_bar = _segment_reduce_raw(_ffi.MP_SUM, gz, ptr1, perm1, self.n)        # adjoint of the sender gather
        if want_wc:
            wc_bar = dense_wgrad(ev, gz, with_bias=False)[0]
        if want_edges:
            e_bar = _dense_raw(gz, wc.t().contiguous(), None, 0, 0.0)
        return pj_bar, pi_bar, e_bar, wc_bar

    def bias_weight(self):
        """``c (N, 1)``: what the pool makes of a constant 1 per edge - the receiver's edge count for a sum, 1 for a mean,
        0 for a receiver without edges.  Cached on the plan, as a 1-tuple like the plan's other entries (what walks them,
        data/packer.py, iterates over the tensors of an entry)."""
        from ...ops.segment import _segment_reduce_raw
        key = ("inorp_bias_weight", self.op)
        hit = self.plan._csr.get(key)
        if hit is None:
            ptr0, perm0, _ = self.plan.csr(0)
            ones = torch.ones((self.e, 1), dtype=torch.float32, device=self.plan.cols.device)
            hit = self.plan._csr[key] = (_segment_reduce_raw(self.op, ones, ptr0, perm0, self.n),)
        return hit[0]


class INorpEdgeStep(GraphBaseLayer):
    r"""The edge step of one INorp block (kgcnn/literature/INorp.py:119-127) around the block's layers:
    ``step([nodes, edges, edge_index])`` returns ``PoolingLocalEdges(GraphMLP([n_out || n_in || edges]))``,
    ``(batch, [N], H2)``.  ``mlp`` is the block's edge ``GraphMLP`` and ``pooling`` its ``PoolingLocalEdges``: the step owns
    no weight of its own.  ``use_fused_step`` (default False): when on, sizes that fit ``fused_step_supported`` take the
    fused route (``fused_step``, decided in ``build``), with and without a tape.  It is off by default because on the
    measured molecule batch the replayed forward and the training step were slower on it."""

    weight_gradients = True   # the fused rule and the Dense rules around it cover W1, b1, W2, b2; so does the sequence

    def __init__(self, mlp=None, pooling=None, edge_mlp_args=None, pooling_args=None, gather_args=None, **kwargs):
        super().__init__(**kwargs)
        gather_args = gather_args or {}
        self.lay_mlp = mlp if mlp is not None else GraphMLP(**(edge_mlp_args or {"units": [64, 32],
                                                                                 "activation": ["relu", "linear"]}))
        self.lay_pool = pooling if pooling is not None else PoolingLocalEdges(**(pooling_args or {}))
        self.lay_gather_in = GatherNodesIngoing(**gather_args)
        self.lay_gather_out = GatherNodesOutgoing(**gather_args)
        self.lay_concat_nodes = LazyConcatenate(axis=-1)
        self.lay_concat_edges = LazyConcatenate(axis=-1)
        self.use_fused_step = False     # the fused route did not win the replayed forward or the step
        self.fused_step = None          # decided in build(): the sizes fit the fused route

    def build(self, input_shape):
        """``input_shape``: ``[nodes (batch, None, F), edges (batch, None, Fe), edge_index]``; builds the edge MLP if
        nobody has (so ``set_weights`` works before a first call) and decides the route."""
        super().build(input_shape)
        f, fe = input_shape[0][-1], input_shape[1][-1]
        mlp = self.lay_mlp
        mlp.ensure_built((None, None, 2 * int(f) + int(fe)))
        plain = not any(mlp._conf_use_normalization) and not any(mlp._conf_use_dropout)
        self.fused_step = bool(fused_step_supported(f, fe, mlp._conf_units, mlp._conf_activation, mlp._conf_use_bias,
                                                    self.lay_pool.pooling_method, self.lay_pool.pooling_index,
                                                    self.dtype, plain))

    def layer_sequence(self, nodes, edges, edge_index, **kwargs):
        """The reference's layers."""
        eu1 = self.lay_gather_in([nodes, edge_index], **kwargs)
        eu2 = self.lay_gather_out([nodes, edge_index], **kwargs)
        upd = self.lay_concat_nodes([eu2, eu1], **kwargs)
        eu = self.lay_mlp(self.lay_concat_edges([upd, edges], **kwargs), **kwargs)
        return self.lay_pool([nodes, eu, edge_index], **kwargs)

    def fused(self, nodes, edges, edge_index):
        """The folded step: three Dense launches on the nodes around ``mp_inorp_edge_f32``."""
        from ...autograd import InorpEdge, needs_grad
        d1, d2 = self.lay_mlp.mlp_dense_layer_list
        nv, ev = nodes.values, edges.values
        spec = EdgeStepSpec(nodes, edges, edge_index, self.lay_mlp.mlp_activation_layer_list[0].activation,
                            self.lay_pool.pooling_method)
        k1 = d1.kernel
        f, fe = (int(nv.shape[1]) if nv.dim() == 2 else -1), spec.fe
        if f < 0 or int(k1.shape[0]) != 2 * f + fe:
            raise ValueError("the fused INorp step: nodes %s and edges %s against a first kernel of %d rows"
                             % (tuple(nv.shape), tuple(ev.shape), int(k1.shape[0])))
        # row blocks of the first kernel, read in place (views: a repacked copy could go stale under graph replay)
        pj = dense_values(nv, k1[:f], None, "linear")
        pi = dense_values(nv, k1[f:2 * f], d1.bias, "linear")
        wc = k1[2 * f:2 * f + fe]
        if needs_grad(pj, pi, ev, wc):
            s = InorpEdge.apply(pj, pi, ev, wc, spec)
        else:
            s = spec.forward(pj.contiguous(), pi.contiguous(), ev.detach().contiguous(), wc.detach())
        nu = dense_values(s, d2.kernel, None, "linear")
        if d2.bias is not None:
            nu = binary_values(_ffi.MP_ADD, nu, binary_values(_ffi.MP_MUL, spec.bias_weight(), d2.bias.view(1, -1)))
        return nodes.with_values(nu)

    def call(self, inputs, **kwargs):
        """inputs: ``[nodes (batch,[N],F), edges (batch,[M],Fe), edge_index (batch,[M],2)]`` -> ``(batch,[N],H2)``."""
        nodes, edges, edge_index = inputs
        if self.fused_step and self.use_fused_step and not kwargs:
            return self.fused(nodes, edges, edge_index)
        return self.layer_sequence(nodes, edges, edge_index, **kwargs)

    def get_config(self):
        config = super().get_config()
        config.update({"edge_mlp_args": self.lay_mlp.get_config(), "pooling_args": self.lay_pool.get_config()})
        return config
