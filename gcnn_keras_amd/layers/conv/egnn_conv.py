"""The fused edge step of an EGNN block (kgcnn/literature/EGNN.py:155-174 without edge attributes) on csrc/mp_egnn.hip.

The reference gathers both end nodes of every edge, concatenates ``[h_i, h_j, enc]``, runs the two Dense layers of the edge
MLP and the one-unit attention Dense on the ``(E, 2F + 2K)`` tensor, multiplies and sums into the receivers.
``FusedEdgeStep`` computes the same sums in three launches: ``Pa = h W_a`` and ``Pb = h W_b`` on the node side
(``mp_dense_f32`` on the first two row blocks of the first Dense kernel, read in place), then ``mp_egnn_edge_f32``, which
gathers one row of each per edge, adds the encoding's product and the bias, runs the second layer on the matrix pipe,
the attention in its epilogue and the per-receiver sums in edge order.  The first layer's summation order differs from
the reference's single 276-term dot product; the result stays in the float32 class.

Served sizes (``FUSED_EDGE_SIZES``): node and message width 128, an edge MLP of exactly two biased or unbiased layers of
128 without normalisation or dropout, an encoding of at most 64 columns (or the bare norm output), sum pooling into index
column 0, activations among the engine's codes, attention absent or one unit.  Everything else takes the layer sequence.

Reverse (forces): ``autograd.EgnnEdge``, first order.  A forward on the tape stores both pre-activations ``z1``, ``z2``
``(E, 128)``; the reverse reads them, runs the mirror GEMM with ``W2^T`` and the activation derivatives, and sums the
first layer's gradient per node over the CSRs of both index columns (``mp_segment_reduce_csr_f32``).  The weights are
read in place and get no gradients: ``weights_need_grad`` tells the builder to step aside to the layer sequence.
"""
import torch

from ... import _ffi

FUSED_EDGE_SIZES = {"units": 128, "max_encoding": 64}   # csrc/mp_egnn.hip


def _plain_mlp(mlp, units):
    """``mlp`` is Dense + activation only, with exactly these units and engine activations."""
    if mlp is None or list(mlp._conf_units) != list(units):
        return False
    if any(mlp._conf_use_normalization) or any(mlp._conf_use_dropout):
        return False
    return all(a.activation in _ffi.ACTIVATION_CODES for a in mlp.mlp_activation_layer_list)


def fused_edge_supported(node_width, edge_mlp, attention_mlp, encoding, pooling_method, pooling_index=0):
    """True when one block's edge step with these layers runs on ``mp_egnn_edge_f32`` (the configuration decides)."""
    s = FUSED_EDGE_SIZES
    if node_width != s["units"] or not _plain_mlp(edge_mlp, [s["units"], s["units"]]):
        return False
    if attention_mlp is not None and not _plain_mlp(attention_mlp, [1]):
        return False
    if encoding is not None and 2 * int(encoding.dim_half) > s["max_encoding"]:
        return False
    return pooling_method in ("sum", "segment_sum", "reduce_sum") and pooling_index == 0


class EdgeStepSpec:
    """One fused edge step bound to an index plan and the (frozen) weights of its block."""

    def __init__(self, plan, step, device):
        self.plan = plan
        d1, d2 = step.edge_mlp.mlp_dense_layer_list
        a1, a2 = step.edge_mlp.mlp_activation_layer_list
        self.wc = d1.kernel.detach()[2 * FUSED_EDGE_SIZES["units"]:]
        self.b1 = None if d1.bias is None else d1.bias.detach()
        self.w2 = d2.kernel.detach()
        self.b2 = None if d2.bias is None else d2.bias.detach()
        self.act1, self.act2 = _ffi.activation_code(a1.activation), _ffi.activation_code(a2.activation)
        self.w_att = self.b_att = None
        self.act_att = 0
        if step.attention_mlp is not None:
            da = step.attention_mlp.mlp_dense_layer_list[0]
            self.w_att = da.kernel.detach().reshape(-1)
            self.b_att = None if da.bias is None else da.bias.detach()
            self.act_att = _ffi.activation_code(step.attention_mlp.mlp_activation_layer_list[0].activation)
        enc = step.encoding
        self.scales = None if enc is None else enc.scales(device)
        self.dim_half = 0 if enc is None else int(enc.dim_half)
        self.interleave = 0 if enc is None else int(bool(enc.interleave_sin_cos))
        self.alpha = 0.05   # leaky_relu slope of layers/modules.py dense_values

    def forward(self, pa, pb, x, save=False):
        n, e, f = self.plan.N, self.plan.M, FUSED_EDGE_SIZES["units"]
        ptr0, perm0, _ = self.plan.csr(0)
        ws, nbytes = _ffi.float_workspace("mp_egnn_edge_ws_bytes", e, device=pa.device)
        out = torch.empty((n, f), dtype=torch.float32, device=pa.device)
        z1 = torch.empty((e, f), dtype=torch.float32, device=pa.device) if save else None
        z2 = torch.empty((e, f), dtype=torch.float32, device=pa.device) if save else None
        _ffi.call("mp_egnn_edge_f32", _ffi.ptr(pa), _ffi.ptr(pb), n, _ffi.ptr(x), _ffi.ptr(self.plan.cols), e,
                  _ffi.ptr(ptr0), _ffi.ptr(perm0), _ffi.ptr(self.scales), self.dim_half, self.interleave, _ffi.ptr(self.wc),
                  _ffi.ptr(self.b1), self.act1, _ffi.ptr(self.w2), _ffi.ptr(self.b2), self.act2, _ffi.ptr(self.w_att),
                  _ffi.ptr(self.b_att), self.act_att, self.alpha, _ffi.ptr(ws), nbytes, _ffi.ptr(z1),
                  _ffi.ptr(z2), _ffi.ptr(out), _ffi.stream())
        return (out, z1, z2) if save else out

    def grad(self, x, z1, z2, g, want_a=True, want_b=True, want_x=True):
        from ...ops.segment import _segment_reduce_raw
        n, e, f = self.plan.N, self.plan.M, FUSED_EDGE_SIZES["units"]
        z1_bar = torch.empty((e, f), dtype=torch.float32, device=x.device)
        x_bar = torch.empty_like(x) if want_x else None
        _ffi.call("mp_egnn_edge_grad_f32", _ffi.ptr(g.contiguous()), n, _ffi.ptr(x), _ffi.ptr(self.plan.cols), e,
                  _ffi.ptr(z1), _ffi.ptr(z2), _ffi.ptr(self.scales), self.dim_half, self.interleave, _ffi.ptr(self.wc),
                  self.act1, _ffi.ptr(self.w2), self.act2, _ffi.ptr(self.w_att), _ffi.ptr(self.b_att), self.act_att,
                  self.alpha, _ffi.ptr(z1_bar), _ffi.ptr(x_bar), _ffi.stream())
        bars = []
        for col, want in ((0, want_a), (1, want_b)):
            if want:
                ptr, perm, _ = self.plan.csr(col)
                bars.append(_segment_reduce_raw(_ffi.MP_SUM, z1_bar, ptr, perm, n, None, False))
            else:
                bars.append(None)
        return bars[0], bars[1], x_bar


class FusedEdgeStep:
    """The edge step of one EGNN block over the block's own layers (``edge_mlp``, ``attention_mlp`` or None,
    ``encoding`` or None): ``step(h, norm_x, edge_index)`` returns the pooled messages ``m_i`` (ragged like ``h``)."""

    def __init__(self, edge_mlp, attention_mlp, encoding):
        self.edge_mlp, self.attention_mlp, self.encoding = edge_mlp, attention_mlp, encoding

    def weight_tensors(self):
        layers = list(self.edge_mlp.mlp_dense_layer_list)
        if self.attention_mlp is not None:
            layers += self.attention_mlp.mlp_dense_layer_list
        return [t for lay in layers for t in (lay.kernel, lay.bias) if t is not None]

    def weights_need_grad(self):
        """The kernel reads the weights in place and has no reverse rule for them (autograd.EgnnEdge)."""
        return torch.is_grad_enabled() and any(t.requires_grad for t in self.weight_tensors())

    def __call__(self, h, norm_x, edge_index):
        from ...autograd import EgnnEdge, needs_grad
        from ..modules import dense_values
        hv, xv = h.values, norm_x.values
        _ffi.require_device(hv, xv, edge_index.values)
        if hv.dtype != torch.float32 or xv.dtype != torch.float32 or xv.dim() != 2 or int(xv.shape[-1]) != 1:
            raise ValueError("the fused EGNN edge step expects float32 nodes and a norm output of shape (batch, [M], 1)")
        plan = edge_index.index_plan(h)
        plan.validate()
        if plan.K != 2 or plan.M != int(xv.shape[0]):
            raise ValueError("the fused EGNN edge step: %d norm rows for %d edges of %d columns"
                             % (int(xv.shape[0]), plan.M, plan.K))
        # row blocks of the first Dense kernel, read in place (views: a repacked copy could go stale under graph replay)
        f = FUSED_EDGE_SIZES["units"]
        kernel = self.edge_mlp.mlp_dense_layer_list[0].kernel.detach()
        pa = dense_values(hv, kernel[:f], None, "linear")
        pb = dense_values(hv, kernel[f:2 * f], None, "linear")
        spec = EdgeStepSpec(plan, self, hv.device)
        if needs_grad(pa, pb, xv):
            return h.with_values(EgnnEdge.apply(pa, pb, xv, spec))
        return h.with_values(spec.forward(pa.contiguous(), pb.contiguous(), xv.contiguous()))
