"""MXMNet layers (mirror of kgcnn/layers/conv/mxmnet_conv.py:11-192) on the HIP engine.

``MXMGlobalMP`` is the global message passing over the range graph, ``MXMLocalMP`` the local one over the bond graph with
its two angle lists.  Both keep the reference's constructor arguments, sub-layer attribute names, op order and
``get_config`` keys, and two of its quirks on purpose:

* ``MXMGlobalMP`` pools with ``PoolingLocalMessages()`` at its default, the **mean**; ``MXMLocalMP`` with its
  ``pooling_method`` (default "sum");
* ``MXMLocalMP`` assigns ``h_mlp`` twice: one ``GraphMLP`` survives and ``call`` uses it twice, so the cross-layer mapping
  and the update function share their weights.  The first ``GraphMLP`` is never called, so it is never built and owns no
  weights, however Keras tracks it; the one that owns them was attached behind ``lin_rbf_out``, so the weights of
  ``h_mlp`` stand between those of ``lin_rbf_out`` and ``y_mlp``.  The second assignment here removes the
  attribute first, which puts the layer at the same place.

Each has two routes, chosen from the configuration in ``build`` and switched by ``use_fused_step`` (and, for the triplet
steps of ``MXMLocalMP``, ``use_fused_triplet``); a call with keyword arguments takes the sequence:

* the *layer sequence*: the reference's ops on the existing engine kernels (gather, concatenate, Dense, multiply, segment
  reduce);
* the *fused route* (csrc/mp_mxmnet.hip).  The Dense on ``[x_i || x_j || a]`` is linear in its three row blocks, so the
  message ``act(Pa[i] + Pb[j] + a Wc + b) * (a Wl)`` is two node-sized Dense launches on row-block views of the kernel
  (read in place) and ONE ``mp_mxm_edge_f32``, which pools it into the receivers and adds the nodes
  (``MXMGlobalMP.propagate``: nothing edge-sized is written) or writes it per edge (``MXMLocalMP``'s ``mlp_kj x lin_rbf1``
  and ``mlp_ji_1``: no ``(E, 2 units + Kr)`` concatenation).  Served: float32, ``units`` in {32, 64, 128}, attribute width
  1 to 128, an activation among the engine's codes.  The triplet steps (gather by angle column 1, multiply with the
  ``mlp_sbf`` rows, pool into angle column 0) are one ``mp_mxm_triplet_f32`` each for sum or mean pooling, any width.

Reverse rules (forces): ``autograd.MxmEdge`` and ``autograd.MxmTriplet``, first order only.  ``ResidualLayer`` carries no
weight gradients, so neither do these (``weight_gradients = False``): inference and forces run, a weight that requires
grad in grad mode raises ``NotImplementedError``.
"""
import torch

from ... import _ffi
from ..base import GraphBaseLayer
from ..gather import GatherEmbeddingSelection, GatherNodesOutgoing
from ..geom import angle_plan
from ..mlp import GraphMLP
from ..modules import Dense, LazyAdd, LazyConcatenate, LazyMultiply, _activation_name, dense_values
from ..pooling import PoolingLocalMessages
from .dimenet_conv import ResidualLayer

FUSED_STEP_SIZES = {"units": (32, 64, 128), "max_edge_width": 128}   # csrc/mp_mxmnet.hip
_FUSED_POOLING = {"mean": _ffi.MP_MEAN, "segment_mean": _ffi.MP_MEAN, "reduce_mean": _ffi.MP_MEAN,
                  "sum": _ffi.MP_SUM, "segment_sum": _ffi.MP_SUM, "reduce_sum": _ffi.MP_SUM}


def fused_step_supported(units, edge_width, activation, pooling_method="sum", dtype="float32"):
    """True when an edge message of these sizes runs on ``mp_mxm_edge_f32`` (the configuration decides)."""
    s = FUSED_STEP_SIZES
    if edge_width is None or dtype not in ("float32", torch.float32):
        return False
    if int(units) not in s["units"] or not 1 <= int(edge_width) <= s["max_edge_width"]:
        return False
    return _activation_name(activation) in _ffi.ACTIVATION_CODES and pooling_method in _FUSED_POOLING


def fused_triplet_supported(pooling_method="sum", dtype="float32"):
    """True when the triplet step runs on ``mp_mxm_triplet_f32``: float32 and sum or mean pooling, any width."""
    return dtype in ("float32", torch.float32) and pooling_method in _FUSED_POOLING


class EdgeMessageSpec:
    """One multiplex edge message bound to an index plan and the frozen weights, for ``autograd.MxmEdge``:
    ``y_e = act(Pa[i_e] + Pb[j_e] + a_e Wc + b) * (a_e Wl)``, pooled into column 0 with ``base`` added
    (``pooling_method`` given) or written per edge (``pooling_method=None``).  ``wc``, ``wl`` (None: no gate) are row
    blocks of the layers' kernels, read in place."""

    def __init__(self, plan, wc, wl, bias, activation, pooling_method=None):
        self.plan = plan
        self.wc, self.wl = wc.detach(), None if wl is None else wl.detach()
        self.bias = None if bias is None else bias.detach()
        self.ka, self.w = int(wc.shape[0]), int(wc.shape[1])
        self.act = _ffi.activation_code(_activation_name(activation))
        self.pooled = pooling_method is not None
        self.op = _FUSED_POOLING[pooling_method] if self.pooled else _ffi.MP_SUM
        self.alpha = 0.05   # leaky_relu slope of layers/modules.py dense_values

    def forward(self, pa, pb, a, base=None, save=False):
        """``out`` (N, W) or ``y`` (E, W) of contiguous values; with ``save`` also the pre-activation and the gate."""
        n, e, w, dev = self.plan.N, self.plan.M, self.w, pa.device
        if int(a.shape[0]) != e or int(a.shape[1]) != self.ka or int(pa.shape[1]) != w or int(pa.shape[0]) != n:
            raise ValueError("the fused MXMNet edge message: projections %s and attributes %s for %d nodes, %d edges and "
                             "a (%d, %d) kernel block" % (tuple(pa.shape), tuple(a.shape), n, e, self.ka, w))
        z = torch.empty((e, w), dtype=torch.float32, device=dev) if save else None
        lg = torch.empty((e, w), dtype=torch.float32, device=dev) if save and self.wl is not None else None
        ptr0 = perm0 = ws = None
        nbytes = 0
        if self.pooled:
            ptr0, perm0, _ = self.plan.csr(0)
            ws, nbytes = _ffi.float_workspace("mp_mxm_edge_ws_bytes", e, w, device=dev)
            res = torch.empty((n, w), dtype=torch.float32, device=dev)
        else:
            res = torch.empty((e, w), dtype=torch.float32, device=dev)
            if e == 0:   # no rows to write (and an empty tensor has no pointer to tell the epilogue by)
                return (res, z, lg) if save else res
        _ffi.call("mp_mxm_edge_f32", _ffi.ptr(pa), _ffi.ptr(pb), n, w, _ffi.ptr(a), self.ka, _ffi.ptr(self.wc),
                  _ffi.ptr(self.wl), _ffi.ptr(self.bias), _ffi.ptr(self.plan.cols), e, _ffi.ptr(ptr0), _ffi.ptr(perm0),
                  self.act, self.alpha, self.op, _ffi.ptr(base), _ffi.ptr(ws), nbytes, _ffi.ptr(z), _ffi.ptr(lg),
                  _ffi.ptr(res) if self.pooled else None, None if self.pooled else _ffi.ptr(res), _ffi.stream())
        return (res, z, lg) if save else res

    def grad(self, z, lg, g, want_pa=True, want_pb=True, want_a=True):
        """``(Pa_bar, Pb_bar, a_bar)`` of the upstream ``g`` ((N, W) pooled, (E, W) per edge)."""
        from ...ops.segment import _segment_reduce_raw
        n, e, w, dev = self.plan.N, self.plan.M, self.w, g.device
        z_bar = torch.empty((e, w), dtype=torch.float32, device=dev)
        a_bar = torch.empty((e, self.ka), dtype=torch.float32, device=dev) if want_a else None
        ptr0 = self.plan.csr(0)[0] if self.pooled else None
        _ffi.call("mp_mxm_edge_grad_f32", _ffi.ptr(g), 1 if self.pooled else 0, n, w, self.ka, _ffi.ptr(self.wc),
                  _ffi.ptr(self.wl), _ffi.ptr(self.plan.cols), e, _ffi.ptr(ptr0), self.act, self.alpha, self.op,
                  _ffi.ptr(z), _ffi.ptr(lg), _ffi.ptr(z_bar), _ffi.ptr(a_bar), _ffi.stream())
        bars = []
        for col, want in ((0, want_pa), (1, want_pb)):
            if want:
                ptr, perm, _ = self.plan.csr(col)
                bars.append(_segment_reduce_raw(_ffi.MP_SUM, z_bar, ptr, perm, n, None, False))
            else:
                bars.append(None)
        return bars[0], bars[1], a_bar


class TripletPoolSpec:
    """The triplet pool bound to an angle plan: ``out[n] = pool_{t: A[t,0] = n} x[A[t,1]] * s[t]``."""

    def __init__(self, plan, pooling_method):
        self.plan, self.op = plan, _FUSED_POOLING[pooling_method]

    def forward(self, x, s):
        e, t, w = self.plan.N, self.plan.M, int(x.shape[1])
        if int(x.shape[0]) != e or tuple(s.shape) != (t, w):
            raise ValueError("the MXMNet triplet pool: messages %s and basis rows %s for %d edges and %d triplets"
                             % (tuple(x.shape), tuple(s.shape), e, t))
        ptr0, perm0, _ = self.plan.csr(0)
        out = torch.empty((e, w), dtype=torch.float32, device=x.device)
        _ffi.call("mp_mxm_triplet_f32", _ffi.ptr(x), e, w, _ffi.ptr(s), _ffi.ptr(self.plan.cols), t, _ffi.ptr(ptr0),
                  _ffi.ptr(perm0), self.op, _ffi.ptr(out), _ffi.stream())
        return out

    def grad(self, x, s, g, want_x=True, want_s=True):
        if not (want_x or want_s):
            return None, None
        e, t, w = self.plan.N, self.plan.M, int(x.shape[1])
        ptr0 = self.plan.csr(0)[0]
        ptr1, perm1, _ = self.plan.csr(1)
        x_bar = torch.empty_like(x) if want_x else None
        s_bar = torch.empty_like(s) if want_s else None
        _ffi.call("mp_mxm_triplet_grad_f32", _ffi.ptr(x), e, w, _ffi.ptr(s), _ffi.ptr(self.plan.cols), t, _ffi.ptr(ptr0),
                  _ffi.ptr(ptr1), _ffi.ptr(perm1), self.op, _ffi.ptr(g.contiguous()), _ffi.ptr(x_bar), _ffi.ptr(s_bar),
                  _ffi.stream())
        return x_bar, s_bar


def _edge_message(layer, x, attr, edge_index, mlp, linear, pooling_method=None, base=None):
    """``mlp([x_i || x_j || attr]) * linear(attr)`` on ``mp_mxm_edge_f32`` for a one-layer ``mlp`` (``linear`` None: no
    gate): two node-sized Dense launches on row blocks of the kernel, read in place (views: a repacked copy could go
    stale under graph replay), then the fused message.  Returns values: (N, W) pooled, (E, W) otherwise."""
    from ...autograd import MxmEdge, needs_grad
    xv, av = x.values, attr.values
    _ffi.require_device(xv, av, edge_index.values)
    plan = edge_index.index_plan(x)
    plan.validate()
    dense = mlp.mlp_dense_layer_list[0]
    kernel, f = dense.kernel.detach(), int(xv.shape[1])
    if xv.dtype != torch.float32 or av.dtype != torch.float32 or av.dim() != 2 or plan.K != 2 \
            or int(av.shape[0]) != plan.M or int(kernel.shape[0]) != 2 * f + int(av.shape[1]):
        raise ValueError("%s: nodes %s and edge attributes %s against a kernel of %d rows over %d edges of %d columns"
                         % (layer.name, tuple(xv.shape), tuple(av.shape), int(kernel.shape[0]), plan.M, plan.K))
    pa = dense_values(xv, kernel[:f], None, "linear")
    pb = dense_values(xv, kernel[f:2 * f], None, "linear")
    spec = EdgeMessageSpec(plan, kernel[2 * f:], None if linear is None else linear.kernel, dense.bias,
                           mlp.mlp_activation_layer_list[0].activation, pooling_method)
    bv = None if base is None else base.values
    if needs_grad(pa, pb, av, bv):
        return MxmEdge.apply(pa, pb, av, bv, spec)
    return spec.forward(pa.contiguous(), pb.contiguous(), av.contiguous(), None if bv is None else bv.contiguous())


class MXMGlobalMP(GraphBaseLayer):
    """Global message passing of MXMNet (kgcnn/layers/conv/mxmnet_conv.py:11-82).  Inputs ``[nodes (batch, [N], F),
    edge_attr (batch, [M], Ka), edge_index (batch, [M], 2)]``; returns the updated nodes ``(batch, [N], units)``."""

    weight_gradients = False   # ResidualLayer has no tested weight gradients

    def __init__(self, units: int = 64, **kwargs):
        super().__init__(**kwargs)
        self.dim = units
        self.h_mlp = GraphMLP(self.dim, activation="swish")
        self.res1 = ResidualLayer(self.dim)
        self.res2 = ResidualLayer(self.dim)
        self.res3 = ResidualLayer(self.dim)
        self.mlp = GraphMLP(self.dim, activation="swish")
        self.add_res = LazyAdd()

        self.x_edge_mlp = GraphMLP(self.dim, activation="swish")
        self.linear = Dense(self.dim, use_bias=False, activation="linear")

        self.gather = GatherEmbeddingSelection([0, 1])
        self.pool = PoolingLocalMessages()
        self.cat = LazyConcatenate()
        self.multiply_edge = LazyMultiply()
        self.add = LazyAdd()
        self.use_fused_step = True      # False: propagate takes the reference's layer sequence
        self.fused_step = None          # decided in build(): the sizes fit mp_mxm_edge_f32

    def build(self, input_shape):
        super().build(input_shape)
        h_shape, a_shape = tuple(input_shape[0]), tuple(input_shape[1])
        lead, dim = h_shape[:-1], self.dim
        self.h_mlp.ensure_built(h_shape)
        for layer in (self.res1, self.res2, self.res3, self.mlp):
            layer.ensure_built(lead + (dim,))
        self.x_edge_mlp.ensure_built(tuple(a_shape[:-1]) + (2 * dim + int(a_shape[-1]),))
        self.linear.ensure_built(a_shape)
        self.fused_step = bool(fused_step_supported(dim, a_shape[-1], "swish", self.pool.pooling_method, self.dtype)
                               and self.pool.pooling_index == 0)

    def propagate(self, edge_index, x, edge_attr, **kwargs):
        """``x + mean_{e: i_e = r} swish([x_i || x_j || a_e] W + b) * (a_e W_l)`` (mxmnet_conv.py:38-53): one
        ``mp_mxm_edge_f32`` behind two node-sized Dense launches on the fused route, else the layer sequence."""
        if self.fused_step and self.use_fused_step and not kwargs:
            return x.with_values(_edge_message(self, x, edge_attr, edge_index, self.x_edge_mlp, self.linear,
                                               self.pool.pooling_method, base=x))
        x_i, x_j = self.gather([x, edge_index])

        # Prepare message.
        x_edge = self.cat([x_i, x_j, edge_attr])
        x_edge = self.x_edge_mlp(x_edge, **kwargs)
        edge_attr_lin = self.linear(edge_attr, **kwargs)
        x_edge = self.multiply_edge([edge_attr_lin, x_edge])

        # Pooling here.
        x_p = self.pool([x, x_edge, edge_index])

        # Replace self loops by explicit node update here.
        return self.add([x_p, x])

    def call(self, inputs, **kwargs):
        h, edge_attr, edge_index = inputs

        # Keep for residual skip connections.
        res_h = h

        # Integrate the Cross Layer Mapping inside the Global Message Passing
        h = self.h_mlp(h)

        # Message Passing operation
        h = self.propagate(edge_index=edge_index, x=h, edge_attr=edge_attr, **kwargs)

        # Update function f_u
        h = self.res1(h)
        h = self.mlp(h)
        h = self.add_res([h, res_h])
        h = self.res2(h)
        h = self.res3(h)

        # Message Passing operation
        return self.propagate(edge_index=edge_index, x=h, edge_attr=edge_attr, **kwargs)

    def get_config(self):
        config = super().get_config()
        config.update({"units": self.dim})
        return config


class MXMLocalMP(GraphBaseLayer):
    """Local message passing of MXMNet (kgcnn/layers/conv/mxmnet_conv.py:85-192).  Inputs ``[nodes (batch, [N], F),
    rbf (batch, [M], Kr), sbf1 (batch, [T1], Ks), sbf2 (batch, [T2], Ks), edge_index (batch, [M], 2),
    angle_index_1 (batch, [T1], 2), angle_index_2 (batch, [T2], 2)]``; returns ``(nodes (batch, [N], units),
    y (batch, [N], output_units))``."""

    weight_gradients = False   # ResidualLayer has no tested weight gradients

    def __init__(self, units: int = 64, output_units: int = 1, activation: str = "swish",
                 output_kernel_initializer: str = "zeros", pooling_method: str = "sum", **kwargs):
        super().__init__(**kwargs)
        self.dim = units
        self.output_dim = output_units
        self.activation = activation
        self.pooling_method = pooling_method
        self.h_mlp = GraphMLP(self.dim, activation=activation)

        self.mlp_kj = GraphMLP([self.dim], activation=activation)
        self.mlp_ji_1 = GraphMLP([self.dim], activation=activation)
        self.mlp_ji_2 = GraphMLP([self.dim], activation=activation)
        self.mlp_jj = GraphMLP([self.dim], activation=activation)

        self.mlp_sbf1 = GraphMLP([self.dim, self.dim], activation=activation)
        self.mlp_sbf2 = GraphMLP([self.dim, self.dim], activation=activation)
        self.lin_rbf1 = Dense(self.dim, use_bias=False, activation="linear")
        self.lin_rbf2 = Dense(self.dim, use_bias=False, activation="linear")

        self.res1 = ResidualLayer(self.dim)
        self.res2 = ResidualLayer(self.dim)
        self.res3 = ResidualLayer(self.dim)

        self.lin_rbf_out = Dense(self.dim, use_bias=False, activation="linear")

        # the reference assigns h_mlp a second time here: the first layer is dropped, this one takes its place in the
        # layer (and weight) order, and call() uses it for both the cross-layer mapping and the update function
        del self.h_mlp
        self.h_mlp = GraphMLP(self.dim, activation=activation)

        self.y_mlp = GraphMLP([self.dim, self.dim, self.dim], activation=activation)
        self.y_W = Dense(self.output_dim, activation="linear", kernel_initializer=output_kernel_initializer)
        self.add_res = LazyAdd()

        self.gather_nodes = GatherEmbeddingSelection([0, 1])
        self.cat = LazyConcatenate()
        self.multiply = LazyMultiply()
        self.gather_mkj = GatherNodesOutgoing()
        self.gather_mjj = GatherNodesOutgoing()
        self.pool_mkj = PoolingLocalMessages(pooling_method=pooling_method)
        self.pool_mjj = PoolingLocalMessages(pooling_method=pooling_method)
        self.pool_h = PoolingLocalMessages(pooling_method=pooling_method)
        self.add_mji_1 = LazyAdd()
        self.add_mji_2 = LazyAdd()
        # at the MD17 configuration the two per-edge messages were slower fused than as the layer sequence
        # (0.68 against 0.66 ms per layer, both runs), so they are off by default; the triplet pools won and are on
        self.use_fused_step = False     # True: mlp_kj x lin_rbf1 and mlp_ji_1 run on mp_mxm_edge_f32
        self.use_fused_triplet = True   # False: both triplet steps take the layer sequence
        self.fused_step = None          # decided in build(): the sizes fit mp_mxm_edge_f32
        self.fused_triplet = None       # decided in build(): the pooling fits mp_mxm_triplet_f32

    def build(self, input_shape):
        super().build(input_shape)
        h_shape, rbf_shape, sbf1_shape, sbf2_shape = [tuple(s) for s in input_shape[:4]]
        dim = self.dim
        if int(h_shape[-1]) != dim:
            # h_mlp maps the input AND the pooled messages (width units): one kernel cannot take two widths
            raise ValueError("%s: the shared h_mlp needs nodes of width units=%d, got %d" % (self.name, dim, h_shape[-1]))
        lead_n, lead_e = h_shape[:-1], rbf_shape[:-1]
        self.h_mlp.ensure_built(h_shape)
        cat_shape = lead_e + (2 * dim + int(rbf_shape[-1]),)
        self.mlp_kj.ensure_built(cat_shape)
        self.mlp_ji_1.ensure_built(cat_shape)
        self.mlp_ji_2.ensure_built(lead_e + (dim,))
        self.mlp_jj.ensure_built(lead_e + (dim,))
        self.mlp_sbf1.ensure_built(sbf1_shape)
        self.mlp_sbf2.ensure_built(sbf2_shape)
        for layer in (self.lin_rbf1, self.lin_rbf2, self.lin_rbf_out):
            layer.ensure_built(rbf_shape)
        for layer in (self.res1, self.res2, self.res3, self.y_mlp):
            layer.ensure_built(lead_n + (dim,))
        self.y_W.ensure_built(lead_n + (dim,))
        self.fused_step = bool(fused_step_supported(dim, rbf_shape[-1], self.activation, "sum", self.dtype))
        self.fused_triplet = bool(fused_triplet_supported(self.pooling_method, self.dtype)
                                  and self.pool_mkj.pooling_index == 0)

    def triplet_step(self, m, sw_sbf, angle_idx, gather, pool, **kwargs):
        """``pool_{t: A[t,0] = n} m[A[t,1]] * sw_sbf[t]`` (mxmnet_conv.py:145-148, :158-161): ``mp_mxm_triplet_f32`` on the
        fused route, else GatherNodesOutgoing / LazyMultiply / PoolingLocalMessages."""
        if self.fused_triplet and self.use_fused_triplet and not kwargs:
            from ...autograd import MxmTriplet, needs_grad
            spec = TripletPoolSpec(angle_plan(angle_idx, m, self), self.pooling_method)
            mv, sv = m.values.contiguous(), sw_sbf.values.contiguous()
            if needs_grad(mv, sv):
                return m.with_values(MxmTriplet.apply(mv, sv, spec))
            return m.with_values(spec.forward(mv, sv))
        m_t = gather([m, angle_idx])
        m_t = self.multiply([m_t, sw_sbf])
        return pool([m, m_t, angle_idx])

    def call(self, inputs, **kwargs):
        h, rbf, sbf1, sbf2, edge_index, angle_idx_1, angle_idx_2 = inputs
        res_h = h

        # Integrate the Cross Layer Mapping inside the Local Message Passing
        h = self.h_mlp(h, **kwargs)

        # Message Passing 1
        sw_sbf1 = self.mlp_sbf1(sbf1, **kwargs)
        if self.fused_step and self.use_fused_step and not kwargs:
            # mlp_kj([h_i || h_j || rbf]) * lin_rbf1(rbf) and mlp_ji_1([h_i || h_j || rbf]): two fused edge messages, no
            # (E, 2 units + Kr) concatenation
            m_kj = rbf.with_values(_edge_message(self, h, rbf, edge_index, self.mlp_kj, self.lin_rbf1))
            m_kj = self.triplet_step(m_kj, sw_sbf1, angle_idx_1, self.gather_mkj, self.pool_mkj)
            m_ji_1 = rbf.with_values(_edge_message(self, h, rbf, edge_index, self.mlp_ji_1, None))
        else:
            hi, hj = self.gather_nodes([h, edge_index])
            m = self.cat([hi, hj, rbf])

            m_kj = self.mlp_kj(m, **kwargs)
            w_rbf1 = self.lin_rbf1(rbf, **kwargs)
            m_kj = self.multiply([m_kj, w_rbf1])
            m_kj = self.triplet_step(m_kj, sw_sbf1, angle_idx_1, self.gather_mkj, self.pool_mkj, **kwargs)

            m_ji_1 = self.mlp_ji_1(m, **kwargs)

        m = self.add_mji_1([m_ji_1, m_kj])

        # Message Passing 2 (index jj denotes j'i in the main paper)
        m_jj = self.mlp_jj(m, **kwargs)
        w_rbf2 = self.lin_rbf2(rbf, **kwargs)
        m_jj = self.multiply([m_jj, w_rbf2])
        sw_sbf2 = self.mlp_sbf2(sbf2, **kwargs)
        m_jj = self.triplet_step(m_jj, sw_sbf2, angle_idx_2, self.gather_mjj, self.pool_mjj, **kwargs)

        m_ji_2 = self.mlp_ji_2(m, **kwargs)

        m = self.add_mji_2([m_ji_2, m_jj])

        # Aggregation
        w_rbf = self.lin_rbf_out(rbf, **kwargs)
        m = self.multiply([w_rbf, m])
        h = self.pool_h([h, m, edge_index])

        # Update function f_u
        h = self.res1(h, **kwargs)
        h = self.h_mlp(h, **kwargs)
        h = self.add_res([h, res_h])
        h = self.res2(h, **kwargs)
        h = self.res3(h, **kwargs)

        # Output Module
        y = self.y_mlp(h, **kwargs)
        y = self.y_W(y, **kwargs)

        return h, y

    def get_config(self):
        config = super().get_config()
        out_conf = self.y_W.get_config()
        config.update({"units": self.dim, "output_units": self.output_dim, "activation": self.activation,
                       "output_kernel_initializer": out_conf["kernel_initializer"],
                       "pooling_method": self.pooling_method})
        return config
