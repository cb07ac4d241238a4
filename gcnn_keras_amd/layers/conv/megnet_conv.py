"""MEGNet block (mirror of kgcnn/layers/conv/megnet_conv.py:10-129): edge, node and graph-state updates of one block,
and the fused edge step on csrc/mp_megnet.hip.

The three updates are three-layer Dense chains on concatenated inputs; the graph state reaches edges and nodes through
``GatherState`` (a per-graph row repeated over the graph's edges / nodes, ``mp_repeat_rows_f32``) and is updated from
the per-graph pools of the new edges and nodes (``mp_pool_graph_f32``).  ``MEGnetBlock.call`` is that op sequence on the
engine's layers (the *layer sequence*: every configuration, all training - every op carries its reverse rule, so
``weight_gradients`` is on).

For the served sizes ``FusedEdgeStep`` computes the edge update and its pool into the receivers in four launches plus a
finishing pass: the products ``v W_e[0:Fn]``, ``v W_e[Fn:2Fn]`` and ``u W_e[2Fn+Fe:] + b`` (``mp_dense_f32`` on row-block
views of the first edge kernel, read in place) and ``mp_megnet_edge_f32``, which gathers one row of each per edge - the
state row through the edge tensor's own ``row_splits`` -, adds the edge features' product, runs the two remaining Dense
layers on the matrix pipe and sums per receiver in list order.  The gather of both end nodes, the state repeat, the
concatenation and the three Dense outputs over edges are never written.  The node chain, the state chain and the two
per-graph pools stay on the layers; they read the new edges and the pool.

Served sizes (``FUSED_EDGE_SIZES``, ``fused_edge_supported``): node, edge and state width 32 (what the blocks of
``literature/Megnet.py`` see behind their feed-forward MLPs), ``edge_embed == [64, 32, 32]``, any activation among the
engine's codes, ``use_bias`` either way, mean or sum pooling, float32.  The fused step is forward-only: a call in grad mode
where an input or a weight requires grad takes the layer sequence, and so do ``layer.use_fused_edge = False`` and any call
with keyword arguments.  Edge lists that are not receiver-sorted are served through the plan's CSR permutation.
"""
import torch

from ... import _ffi
from ..base import GraphBaseLayer
from ..gather import GatherNodes, GatherState
from ..modules import Dense, LazyConcatenate, _activation_name
from ..pooling import PoolingGlobalEdges, PoolingLocalEdges, PoolingNodes

_KERNEL_KEYS = ("kernel_regularizer", "activity_regularizer", "bias_regularizer", "kernel_constraint", "bias_constraint",
                "kernel_initializer", "bias_initializer")

FUSED_EDGE_SIZES = {"node_width": 32, "edge_width": 32, "state_width": 32, "edge_embed": [64, 32, 32]}   # csrc/mp_megnet.hip
_FUSED_POOLING = {"mean": _ffi.MP_MEAN, "segment_mean": _ffi.MP_MEAN, "reduce_mean": _ffi.MP_MEAN,
                  "sum": _ffi.MP_SUM, "segment_sum": _ffi.MP_SUM, "reduce_sum": _ffi.MP_SUM}


def fused_edge_supported(node_width, edge_width, state_width, edge_embed, activation, pooling_method, dtype="float32"):
    """True when the edge update of one ``MEGnetBlock`` with these sizes runs on ``mp_megnet_edge_f32`` (the
    configuration decides)."""
    s = FUSED_EDGE_SIZES
    if (node_width, edge_width, state_width) != (s["node_width"], s["edge_width"], s["state_width"]):
        return False
    if edge_embed is None or [int(w) for w in edge_embed] != s["edge_embed"]:
        return False
    if _activation_name(activation) not in _ffi.ACTIVATION_CODES:
        return False
    if dtype not in ("float32", torch.float32):
        return False
    return pooling_method in _FUSED_POOLING


class FusedEdgeStep:
    """The edge update of one ``MEGnetBlock`` on ``mp_megnet_edge_f32``: ``step(node, edge, edge_index, env)`` returns
    the new edges and their pool into the receivers."""

    def __init__(self, layer):
        self.layer = layer

    def weight_tensors(self):
        """Kernels and biases of the block's nine Dense layers (its only weights), read off the attributes: this runs on
        every call."""
        lay = self.layer
        out = []
        for d in (lay.lay_phi_n, lay.lay_phi_n_1, lay.lay_phi_n_2, lay.lay_phi_e, lay.lay_phi_e_1, lay.lay_phi_e_2,
                  lay.lay_phi_u, lay.lay_phi_u_1, lay.lay_phi_u_2):
            out += [d.kernel, d.bias]
        return out

    def needs_grad(self, *inputs):
        """The kernel reads the weights in place and has no reverse rule: any tape steps aside to the layer sequence."""
        if not torch.is_grad_enabled():
            return False
        from ...autograd import needs_grad
        return needs_grad(*inputs) or needs_grad(*self.weight_tensors())

    def __call__(self, node, edge, edge_index, env):
        from ..modules import dense_values
        lay = self.layer
        s = FUSED_EDGE_SIZES
        fn, fe, fu = s["node_width"], s["edge_width"], s["state_width"]
        vv, ev = node.values, edge.values
        _ffi.require_device(vv, ev, env, edge_index.values, edge.row_splits)
        if any(t.dtype != torch.float32 for t in (vv, ev, env)) or vv.dim() != 2 or ev.dim() != 2 or env.dim() != 2:
            raise ValueError("the fused MEGNet edge step expects float32 nodes (batch, [N], 32), edges (batch, [M], 32) "
                             "and a state (batch, 32)")
        plan = edge_index.index_plan(node)
        plan.validate()
        n, e, g = plan.N, plan.M, edge.nrows()
        if plan.K != 2 or e != int(ev.shape[0]) or (int(vv.shape[1]), int(ev.shape[1]), int(env.shape[1])) != (fn, fe, fu):
            raise ValueError("the fused MEGNet edge step: %d edge rows for %d edges of %d columns, widths %d / %d / %d"
                             % (int(ev.shape[0]), e, plan.K, int(vv.shape[1]), int(ev.shape[1]), int(env.shape[1])))
        if g != int(env.shape[0]) or g != edge_index.nrows():
            raise ValueError("the fused MEGNet edge step: %d state rows, %d edge lists and %d index lists"
                             % (int(env.shape[0]), g, edge_index.nrows()))
        if n >= 2 ** 31 - 1 or e >= 2 ** 31 - 32:
            raise ValueError("the fused MEGNet edge step indexes nodes and edges with 32 bits")
        # row blocks of the first edge kernel, read in place (views: a repacked copy could go stale under graph replay)
        d0, d1, d2 = lay.lay_phi_e, lay.lay_phi_e_1, lay.lay_phi_e_2
        k0 = d0.kernel.detach()
        detach = lambda t: None if t is None else t.detach()
        act = d0.activation
        vc = vv.detach().contiguous()
        pa = dense_values(vc, k0[:fn], None, "linear")
        pb = dense_values(vc, k0[fn:2 * fn], None, "linear")
        pu = dense_values(env.detach().contiguous(), k0[2 * fn + fe:], detach(d0.bias), "linear")
        ptr0, perm0, _ = plan.csr(0)
        ws, nbytes = _ffi.float_workspace("mp_megnet_edge_ws_bytes", e, device=vv.device)
        e_out = torch.empty((e, s["edge_embed"][2]), dtype=torch.float32, device=vv.device)
        pool = torch.empty((n, s["edge_embed"][2]), dtype=torch.float32, device=vv.device)
        _ffi.call("mp_megnet_edge_f32", _ffi.ptr(pa), _ffi.ptr(pb), n, _ffi.ptr(pu), _ffi.ptr(edge.row_splits), g,
                  _ffi.ptr(ev.detach().contiguous()), fn, fe, fu, _ffi.ptr(plan.cols), e, _ffi.ptr(ptr0), _ffi.ptr(perm0),
                  _ffi.ptr(k0[2 * fn:2 * fn + fe]), _ffi.ptr(d1.kernel.detach()), _ffi.ptr(detach(d1.bias)),
                  _ffi.ptr(d2.kernel.detach()), _ffi.ptr(detach(d2.bias)), *s["edge_embed"], _ffi.activation_code(act),
                  0.05, _FUSED_POOLING[lay.pooling_method], _ffi.ptr(ws), nbytes, _ffi.ptr(e_out), _ffi.ptr(pool),
                  _ffi.stream())
        return edge.with_values(e_out), node.with_values(pool)


class MEGnetBlock(GraphBaseLayer):
    r"""One MEGNet block (kgcnn/layers/conv/megnet_conv.py:10-129): ``block([nodes, edges, edge_index, state])`` returns
    the updated ``(nodes, edges, state)``.  ``use_fused_edge`` (default True): sizes that fit ``fused_edge_supported``
    run the edge update and its receiver pool on the fused kernel outside a tape (``fused_edge``, decided in ``build``)."""

    # no weight of this block is left off the tape: GatherNodes, GatherState, LazyConcatenate, Dense and the three
    # poolings carry their rules
    weight_gradients = True

    def __init__(self, node_embed=None, edge_embed=None, env_embed=None, pooling_method="mean", use_bias=True,
                 activation="kgcnn>softplus2", kernel_regularizer=None, bias_regularizer=None, activity_regularizer=None,
                 kernel_constraint=None, bias_constraint=None, kernel_initializer="glorot_uniform",
                 bias_initializer="zeros", **kwargs):
        super().__init__(**kwargs)
        scope = locals()
        kernel_args = {key: scope[key] for key in _KERNEL_KEYS}
        kernel_args["use_bias"] = use_bias
        self.pooling_method = pooling_method
        self.node_embed = list(node_embed) if node_embed is not None else [16, 16, 16]
        self.edge_embed = list(edge_embed) if edge_embed is not None else [16, 16, 16]
        self.env_embed = list(env_embed) if env_embed is not None else [16, 16, 16]
        self.use_bias = use_bias

        def chain(widths):
            return [Dense(units=widths[0], activation=activation, **kernel_args),
                    Dense(units=widths[1], activation=activation, **kernel_args),
                    Dense(units=widths[2], activation="linear", **kernel_args)]

        # attribute order = weight order of the reference (node, edge, environment chains)
        self.lay_phi_n, self.lay_phi_n_1, self.lay_phi_n_2 = chain(self.node_embed)
        self.lay_esum = PoolingLocalEdges(pooling_method=pooling_method)
        self.lay_gather_un = GatherState()
        self.lay_conc_nu = LazyConcatenate(axis=-1)
        self.lay_phi_e, self.lay_phi_e_1, self.lay_phi_e_2 = chain(self.edge_embed)
        self.lay_gather_n = GatherNodes()
        self.lay_gather_ue = GatherState()
        self.lay_conc_enu = LazyConcatenate(axis=-1)
        self.lay_usum_e = PoolingGlobalEdges(pooling_method=pooling_method)
        self.lay_usum_n = PoolingNodes(pooling_method=pooling_method)
        self.lay_conc_u = LazyConcatenate(axis=-1)
        self.lay_phi_u, self.lay_phi_u_1, self.lay_phi_u_2 = chain(self.env_embed)
        self.use_fused_edge = True
        self._fused_step = FusedEdgeStep(self)
        self.fused_edge = None      # decided in build(): the sizes fit the fused kernel

    def build(self, input_shape):
        """Weights of the three Dense chains (so ``set_weights`` works before a first call): the edge chain reads
        [n_i || n_j, e, u], the node chain [pooled e', n, u], the state chain [pooled e', pooled n', u]."""
        super().build(input_shape)
        fn, fe, fu = int(input_shape[0][-1]), int(input_shape[1][-1]), int(input_shape[3][-1])

        def build_chain(layers, widths, in_dim):
            for lay, w in zip(layers, widths):
                lay.ensure_built((None, None, in_dim))
                in_dim = w

        build_chain((self.lay_phi_e, self.lay_phi_e_1, self.lay_phi_e_2), self.edge_embed, 2 * fn + fe + fu)
        build_chain((self.lay_phi_n, self.lay_phi_n_1, self.lay_phi_n_2), self.node_embed, self.edge_embed[-1] + fn + fu)
        build_chain((self.lay_phi_u, self.lay_phi_u_1, self.lay_phi_u_2), self.env_embed,
                    self.edge_embed[-1] + self.node_embed[-1] + fu)
        self.fused_edge = fused_edge_supported(fn, fe, fu, self.edge_embed, self.lay_phi_e.activation,
                                               self.pooling_method, self.dtype)

    @staticmethod
    def _run(layers, x, **kwargs):
        for lay in layers:
            x = lay(x, **kwargs)
        return x

    def call(self, inputs, **kwargs):
        """inputs: ``[nodes (batch,[N],F), edges (batch,[M],Fe), edge_index (batch,[M],2), state (batch,Fu)]`` ->
        ``(nodes, edges, state)`` updated."""
        node, edge, edge_index, env = inputs
        if (self.fused_edge and self.use_fused_edge and not kwargs
                and not self._fused_step.needs_grad(node.values, edge.values, env)):
            # edge update and its pool into the receivers in one kernel (csrc/mp_megnet.hip)
            ep, vb = self._fused_step(node, edge, edge_index, env)
        else:
            # edge update: phi_e([n_i || n_j, e_ij, u])
            e_n = self.lay_gather_n([node, edge_index], **kwargs)
            e_u = self.lay_gather_ue([env, edge], **kwargs)
            ep = self._run((self.lay_phi_e, self.lay_phi_e_1, self.lay_phi_e_2),
                           self.lay_conc_enu([e_n, edge, e_u], **kwargs), **kwargs)
            vb = self.lay_esum([node, ep, edge_index], **kwargs)
        # node update: phi_n([pool_i e'_ij, n_i, u])
        v_u = self.lay_gather_un([env, node], **kwargs)
        vp = self._run((self.lay_phi_n, self.lay_phi_n_1, self.lay_phi_n_2),
                       self.lay_conc_nu([vb, node, v_u], **kwargs), **kwargs)
        # state update: phi_u([pool e', pool n', u])
        es = self.lay_usum_e(ep, **kwargs)
        vs = self.lay_usum_n(vp, **kwargs)
        up = self._run((self.lay_phi_u, self.lay_phi_u_1, self.lay_phi_u_2),
                       self.lay_conc_u([es, vs, env], **kwargs), **kwargs)
        return vp, ep, up

    def get_config(self):
        config = super().get_config()
        config.update({"pooling_method": self.pooling_method, "node_embed": self.node_embed, "use_bias": self.use_bias,
                       "edge_embed": self.edge_embed, "env_embed": self.env_embed})
        dense = self.lay_phi_n.get_config()
        config.update({key: dense[key] for key in _KERNEL_KEYS + ("activation",)})
        return config
