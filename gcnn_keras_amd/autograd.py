"""Reverse-mode rules for the engine ops, used by ``EnergyForceModel`` (kgcnn/model/force.py:159-186) and for training.

``torch.autograd`` supplies the tape (plumbing); every forward AND backward computation is an engine kernel:
gather-backward = segment-sum over the CSR of the gathered index column, segment-sum-backward = gather by the receiver
ids, Dense-backward = Dense with the transposed kernel, plus the elementwise derivative kernels of csrc/mp_backward.hip.
Weight gradients (training, ``Model.train_on_batch``) come from csrc/mp_wgrad.hip: dW = x^T g and db = sum_r g for
Dense, the embedding table gradient, and the reverse of the row softmax.  Each is produced only when
``ctx.needs_input_grad`` asks for it.

Second order (a loss on forces, ``EnergyForceModel.train_on_batch``): a backward that runs in grad mode
(``torch.autograd.grad(E, x, create_graph=True)``) records itself on the tape.  The rules of the SchNet force path do so
through the ``*Adjoint`` functions below, whose forward is the first-order computation and whose backward is its reverse:
a gather for a segment sum and back, the Dense GEMMs and wgrad, and the elementwise second derivatives of
csrc/mp_backward2.hip.  In no-grad mode (every inference tape, every loss on the outputs alone) each rule runs the same
kernels as before.  The other rules are ``once_differentiable``: differentiating them twice raises.
"""
import contextlib

import torch
from torch.autograd.function import once_differentiable

from . import _ffi

_input_grads_only = [False]


@contextlib.contextmanager
def input_grads_only():
    """Inside, the rules skip the gradients of their weights (``EnergyForceModel``'s force pass asks for dE/dx alone,
    while torch still marks every Dense kernel as needing a gradient)."""
    prev = _input_grads_only[0]
    _input_grads_only[0] = True
    try:
        yield
    finally:
        _input_grads_only[0] = prev


def needs_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and torch.is_tensor(t) and t.requires_grad for t in tensors)


def route_weights_need_grad(route):
    """A fused route reads the weights in place and has no reverse rule for them: in grad mode it steps aside as soon as
    one of them requires grad (``route._tensors()`` / the cached ``route._wlist`` of ``_sync_weights``)."""
    if not torch.is_grad_enabled():
        return False
    from .layers.base import weight_epoch
    wl = route._wlist
    if wl is None or route._wepoch != weight_epoch():
        wl = [t for t in route._tensors().values() if t is not None]
    for t in wl:
        if t.requires_grad:
            return True
    return False


def _rows_elems(t):
    rows = int(t.shape[0])
    elems = 1
    for d in t.shape[1:]:
        elems *= int(d)
    return rows, max(elems, 1)


class GatherRows(torch.autograd.Function):
    """rows of ``values`` at plan columns ``colsel`` -> (M, len(colsel), ...)."""

    @staticmethod
    def forward(ctx, values, plan, colsel):
        from .layers.gather import _gather_rows_raw
        ctx.plan, ctx.colsel, ctx.shape = plan, tuple(colsel), tuple(values.shape)
        return _gather_rows_raw(values, plan, colsel)

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():
            return GatherRowsAdjoint.apply(g, ctx.plan, ctx.colsel, ctx.shape), None, None
        return _gather_rows_adjoint(g, ctx.plan, ctx.colsel, ctx.shape), None, None


def _gather_rows_adjoint(g, plan, colsel, shape):
    """Reverse of GatherRows: per gathered column, the CSR segment sum of its slice of ``g``."""
    from .ops.segment import _segment_reduce_raw
    total = None
    for j, col in enumerate(colsel):
        ptr, perm, _ = plan.csr(col)
        gj = g[:, j].contiguous()
        part = _segment_reduce_raw(_ffi.MP_SUM, gj, ptr, perm, plan.N, None, False)
        if total is None:
            total = part
        else:
            from .layers.modules import _binary_raw
            total = _binary_raw(_ffi.MP_ADD, total, part)
    return total.view(shape)


class GatherRowsAdjoint(torch.autograd.Function):
    """GatherRows' backward as a differentiable op of ``g``; its own backward is the gather again."""

    @staticmethod
    def forward(ctx, g, plan, colsel, shape):
        ctx.plan, ctx.colsel = plan, colsel
        return _gather_rows_adjoint(g, plan, colsel, shape)

    @staticmethod
    def backward(ctx, h):
        return GatherRows.apply(h.contiguous(), ctx.plan, ctx.colsel), None, None, None


class SegmentSum(torch.autograd.Function):
    """CSR segment sum / mean (weights, if any, are constants)."""

    @staticmethod
    def forward(ctx, data, op, ptr, perm, n_out, weight, seg_ids):
        from .ops.segment import _segment_reduce_raw
        if op not in (_ffi.MP_SUM, _ffi.MP_MEAN):
            raise NotImplementedError("gradients are implemented for sum / mean pooling")
        ctx.op, ctx.ptr, ctx.perm, ctx.n_out, ctx.weight, ctx.seg_ids = op, ptr, perm, n_out, weight, seg_ids
        ctx.shape = tuple(data.shape)
        return _segment_reduce_raw(op, data, ptr, perm, n_out, weight, False)

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():
            out = SegmentSumAdjoint.apply(g, ctx.op, ctx.ptr, ctx.perm, ctx.n_out, ctx.weight, ctx.seg_ids)
        else:
            out = _segment_sum_adjoint(g, ctx.op, ctx.ptr, ctx.n_out, ctx.weight, ctx.seg_ids)
        return out, None, None, None, None, None, None


def _segment_sum_adjoint(g, op, ptr, n_out, weight, seg_ids):
    """Reverse of SegmentSum: ``g`` gathered by the segment id of every row (divided by the count for the mean, times
    the row weight)."""
    gc = g.contiguous()
    rows, elems = _rows_elems(gc)
    m = int(seg_ids.numel())
    if op == _ffi.MP_MEAN:
        cnt = (ptr[1:n_out + 1] - ptr[:n_out]).to(torch.float32).clamp(min=1.0)
        from .layers.modules import _binary_raw
        gc = _binary_raw(_ffi.MP_MUL, gc.view(rows, elems), (1.0 / cnt).view(rows, 1)).view(gc.shape)
    out = torch.empty((m,) + tuple(gc.shape[1:]), dtype=torch.float32, device=gc.device)
    _ffi.call("mp_gather_rows_f32", _ffi.ptr(gc), rows, elems, _ffi.ptr(seg_ids.contiguous()), m, 1,
              _ffi.int32_array([0]), _ffi.ptr(out), _ffi.stream())
    if weight is not None:
        from .layers.modules import _binary_raw
        out = _binary_raw(_ffi.MP_MUL, out.view(m, elems), weight.contiguous().view(m, 1)).view(out.shape)
    return out


class SegmentSumAdjoint(torch.autograd.Function):
    """SegmentSum's backward (gather by segment id) as a differentiable op of ``g``; its backward is the CSR segment sum."""

    @staticmethod
    def forward(ctx, g, op, ptr, perm, n_out, weight, seg_ids):
        ctx.args = (op, ptr, perm, n_out, weight, seg_ids)
        return _segment_sum_adjoint(g, op, ptr, n_out, weight, seg_ids)

    @staticmethod
    def backward(ctx, h):
        return (SegmentSum.apply(h.contiguous(), *ctx.args),) + (None,) * 6


class WeightedSegmentSum(torch.autograd.Function):
    """CSR segment sum ``out[n] = sum_e w_e data[e]`` with a differentiable weight (attention pooling): the data gradient
    is ``SegmentSum``'s adjoint, the weight gradient ``w_bar_e = g[seg(e)] . data[e]`` (mp_segment_weight_grad_f32).
    First order."""

    @staticmethod
    def forward(ctx, data, weight, ptr, perm, n_out, seg_ids):
        from .ops.segment import _segment_reduce_raw
        ctx.ptr, ctx.n_out, ctx.seg_ids = ptr, n_out, seg_ids
        ctx.save_for_backward(data, weight)
        return _segment_reduce_raw(_ffi.MP_SUM, data, ptr, perm, n_out, weight, False)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        data, weight = ctx.saved_tensors
        gc = g.contiguous()
        d_bar = w_bar = None
        if ctx.needs_input_grad[0]:
            d_bar = _segment_sum_adjoint(gc, _ffi.MP_SUM, ctx.ptr, ctx.n_out, weight, ctx.seg_ids)
        if ctx.needs_input_grad[1]:
            dc = data.contiguous()
            m, elems = _rows_elems(dc)
            w_bar = torch.empty(tuple(weight.shape), dtype=torch.float32, device=gc.device)
            _ffi.call("mp_segment_weight_grad_f32", _ffi.ptr(gc), _ffi.ptr(dc), m, elems,
                      _ffi.ptr(ctx.seg_ids.contiguous()), ctx.n_out, _ffi.ptr(w_bar), _ffi.stream())
        return d_bar, w_bar, None, None, None, None


class SegmentSoftmax(torch.autograd.Function):
    """``segment_softmax`` over CSR segments; backward ``y (g - sum_seg y g)`` (mp_segment_softmax_csr_grad_f32).
    First order."""

    @staticmethod
    def forward(ctx, data, ptr, perm, n_seg):
        from .ops.segment import _segment_softmax_raw
        y = _segment_softmax_raw(data, ptr, perm, n_seg)
        ctx.ptr, ctx.perm, ctx.n_seg = ptr, perm, n_seg
        ctx.save_for_backward(y)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        y, = ctx.saved_tensors
        gc = g.contiguous()
        m, elems = _rows_elems(y)
        # rows outside every segment keep the zero: the softmax does not write them either
        out = torch.zeros_like(y)
        _ffi.call("mp_segment_softmax_csr_grad_f32", _ffi.ptr(y), _ffi.ptr(gc), m, elems, _ffi.ptr(ctx.ptr),
                  _ffi.ptr(ctx.perm), ctx.n_seg, _ffi.ptr(out), _ffi.stream())
        return out, None, None, None


class PoolGraph(torch.autograd.Function):
    """Per-graph sum / mean; backward repeats the graph row over its nodes (GatherState kernel)."""

    @staticmethod
    def forward(ctx, values, op, row_splits, g_rows):
        if op not in (_ffi.MP_SUM, _ffi.MP_MEAN):
            raise NotImplementedError("gradients are implemented for sum / mean pooling")
        ctx.op, ctx.splits, ctx.g, ctx.n = op, row_splits, g_rows, int(values.shape[0])
        rows, elems = _rows_elems(values)
        out = torch.empty((g_rows,) + tuple(values.shape[1:]), dtype=torch.float32, device=values.device)
        _ffi.call("mp_pool_graph_f32", op, _ffi.ptr(values.contiguous()), _ffi.ptr(row_splits), g_rows, elems, None,
                  _ffi.ptr(out), _ffi.stream())
        return out

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():
            return PoolGraphAdjoint.apply(g, ctx.op, ctx.splits, ctx.g, ctx.n), None, None, None
        return _pool_graph_adjoint(g, ctx.op, ctx.splits, ctx.g, ctx.n), None, None, None


def _pool_graph_adjoint(g, op, splits, g_rows, n):
    """Reverse of PoolGraph: every graph row repeated over its nodes (divided by the node count for the mean)."""
    gc = g.contiguous()
    _, elems = _rows_elems(gc)
    if op == _ffi.MP_MEAN:
        cnt = (splits[1:] - splits[:-1]).to(torch.float32).clamp(min=1.0)
        from .layers.modules import _binary_raw
        gc = _binary_raw(_ffi.MP_MUL, gc.view(g_rows, elems), (1.0 / cnt).view(g_rows, 1)).view(gc.shape)
    out = torch.empty((n,) + tuple(gc.shape[1:]), dtype=torch.float32, device=gc.device)
    _ffi.call("mp_repeat_rows_f32", _ffi.ptr(gc), _ffi.ptr(splits), g_rows, elems, n, _ffi.ptr(out), _ffi.stream())
    return out


class PoolGraphAdjoint(torch.autograd.Function):
    """PoolGraph's backward (repeat rows) as a differentiable op of ``g``; its backward is the pooling again."""

    @staticmethod
    def forward(ctx, g, op, splits, g_rows, n):
        ctx.args = (op, splits, g_rows)
        return _pool_graph_adjoint(g, op, splits, g_rows, n)

    @staticmethod
    def backward(ctx, h):
        return PoolGraph.apply(h.contiguous(), *ctx.args), None, None, None, None


def dense_wgrad(x, g, with_bias=True):
    """``(x^T g, sum_r g)`` over the rows of ``x`` (..., K) and ``g`` (..., U) on ``mp_dense_wgrad_f32``."""
    k, u = int(x.shape[-1]), int(g.shape[-1])
    xc, gc = x.contiguous(), g.contiguous()
    rows = xc.numel() // max(k, 1)
    dw = torch.empty((k, u), dtype=torch.float32, device=g.device)
    db = torch.empty((u,), dtype=torch.float32, device=g.device) if with_bias else None
    ws, nbytes = _ffi.float_workspace("mp_dense_wgrad_ws_bytes", rows, k, u, device=g.device, none_if_empty=True)
    _ffi.call("mp_dense_wgrad_f32", _ffi.ptr(xc), rows, k, _ffi.ptr(gc), u, _ffi.ptr(dw), _ffi.ptr(db), _ffi.ptr(ws),
              nbytes, _ffi.stream())
    return dw, db


class Dense(torch.autograd.Function):
    """y = act(x W + b); backward gp = dy * act'(pre), dx = gp W^T, dW = x^T gp, db = sum_rows gp (each only when asked).
    In grad mode the backward is ``DenseAdjoint``, a differentiable op of (dy, x, W, b)."""

    @staticmethod
    def forward(ctx, x, kernel, bias, act_code, alpha):
        from .layers.modules import _dense_raw
        pre = _dense_raw(x, kernel, bias, 0, 0.0)
        ctx.kernel, ctx.bias, ctx.act, ctx.alpha = kernel, bias, act_code, alpha
        # x: for dW, and for the second-order terms of a backward in grad mode (dx_bar through pre needs no x, but dW_bar
        # and the dW rows of the adjoint do)
        ctx.x = x if (ctx.needs_input_grad[1] or ctx.needs_input_grad[0]) else None
        if act_code == 0:
            ctx.pre = None
            return pre
        ctx.pre = pre
        out = torch.empty_like(pre)
        _ffi.call("mp_activation_f32", act_code, float(alpha), _ffi.ptr(pre), pre.numel(), _ffi.ptr(out), _ffi.stream())
        return out

    @staticmethod
    def backward(ctx, g):
        want_x = ctx.needs_input_grad[0]
        want_w = ctx.needs_input_grad[1] and not _input_grads_only[0]
        want_b = ctx.needs_input_grad[2] and not _input_grads_only[0]
        if torch.is_grad_enabled():
            gx, gw, gb = DenseAdjoint.apply(g, ctx.x, ctx.kernel, ctx.bias, ctx.pre, ctx.act, ctx.alpha, want_x, want_w,
                                            want_b)
            return gx, gw, gb, None, None
        gx, gw, gb, _ = _affine_backward(_dense_ops(), g.contiguous(), ctx.x, ctx.kernel, ctx.pre, ctx.act, ctx.alpha,
                                         want_x, want_w, want_b)
        return gx, gw, gb, None, None


def _sum_rows(g):
    u = int(g.shape[-1])
    out = torch.empty((u,), dtype=torch.float32, device=g.device)
    _ffi.call("mp_sum_axis_f32", _ffi.ptr(g), 1, g.numel() // max(u, 1), u, 1, _ffi.ptr(out), _ffi.stream())
    return out


def _dense_ops():
    """The three operations the affine rules below are written in, for Dense: ``affine(x, W, b) = x W (+ b)``,
    ``affine_t(g, W) = g W^T`` and ``wgrad(x, g, with_kernel, with_bias) = (x^T g, sum_rows g)``."""
    from .layers.modules import _dense_raw

    def affine(x, w, b):
        return _dense_raw(x, w, b, 0, 0.0)

    def affine_t(g, w):
        return _dense_raw(g, w.t().contiguous(), None, 0, 0.0)   # (units, in): layout change only

    def wgrad(x, g, with_kernel=True, with_bias=True):
        if with_kernel:
            return dense_wgrad(x, g, with_bias=with_bias)
        return None, _sum_rows(g)

    return affine, affine_t, wgrad


def _relational_ops(rel, nrel):
    """The same three operations with one kernel per relation (``W[rel]``), for RelationalDense."""
    from .layers.relational import relational_dense_raw, relational_dense_t_raw, relational_wgrad

    def affine(x, w, b):
        return relational_dense_raw(x, w, b, rel, 0, 0.0)[1]

    def affine_t(g, w):
        return relational_dense_t_raw(g, w.contiguous(), rel)

    def wgrad(x, g, with_kernel=True, with_bias=True):
        return relational_wgrad(x, g, rel, nrel, with_kernel=with_kernel, with_bias=with_bias)

    return affine, affine_t, wgrad


def _affine_backward(ops, gc, x, kernel, pre, act, alpha, want_x, want_w, want_b):
    """First-order backward of y = act(x W + b) in the operations ``ops``: (dx, dW, db, gp) with gp = dy * act'(pre)."""
    _, affine_t, wgrad = ops
    if pre is not None:
        gp = torch.empty_like(gc)
        _ffi.call("mp_activation_grad_f32", act, float(alpha), _ffi.ptr(pre), _ffi.ptr(gc), gc.numel(), _ffi.ptr(gp),
                  _ffi.stream())
        gc = gp
    gx = gw = gb = None
    if want_x:
        gx = affine_t(gc, kernel)
    if want_w or want_b:
        gw, gb = wgrad(x, gc, with_kernel=want_w, with_bias=want_b)
    return gx, gw, gb, gc


def _affine_adjoint_backward(ops, ctx, hx, hw, hb):
    """Reverse of ``_affine_backward`` as an op of (dy, x, W, b): ``(dy_bar, x_bar, W_bar, b_bar)`` for the upstreams
    hx, hW, hb on dx, dW, db, or None when none of them arrived (the mathematics: ``DenseAdjoint``)."""
    from .layers.modules import _binary_raw
    affine, affine_t, wgrad = ops
    need_g, need_x, need_w, need_b = ctx.needs_input_grad[:4]
    x, kernel, pre, gp = ctx.x, ctx.kernel, ctx.pre, ctx.gp
    u = int(kernel.shape[-1])
    h_gp = None
    if hx is not None:
        h_gp = affine(hx.contiguous(), kernel, None)
    if hw is not None:
        h_gp = _add(h_gp, affine(x, hw.contiguous(), hb.contiguous() if hb is not None else None))
    elif hb is not None:
        rows = gp.numel() // max(u, 1)
        zero = torch.zeros((rows, u), dtype=torch.float32, device=gp.device)
        h_gp = _add(h_gp, _binary_raw(_ffi.MP_ADD, zero, hb.contiguous().view(1, u)).view(gp.shape))
    if h_gp is None:
        return None
    g_bar = pre_bar = None
    if pre is None:
        g_bar = h_gp if need_g else None      # linear: act'' = 0, no pre-activation term
    else:
        if need_g:
            g_bar = torch.empty_like(h_gp)
        if need_x or need_w or need_b:
            pre_bar = torch.empty_like(h_gp)
        _ffi.call("mp_activation_grad2_f32", ctx.act, float(ctx.alpha), _ffi.ptr(pre), _ffi.ptr(ctx.g),
                  _ffi.ptr(h_gp), _ffi.ptr(pre_bar), _ffi.ptr(g_bar), h_gp.numel(), _ffi.stream())
    x_bar = w_bar = b_bar = None
    if need_x:
        if hw is not None:
            x_bar = affine_t(gp, hw)
        if pre_bar is not None:
            x_bar = _add(x_bar, affine_t(pre_bar, kernel))
    if need_w:
        if hx is not None:
            w_bar = wgrad(hx, gp, with_bias=False)[0]
        if pre_bar is not None:
            w_pre, b_bar = wgrad(x, pre_bar, with_bias=need_b)
            w_bar = _add(w_bar, w_pre)
    if need_b and b_bar is None and pre_bar is not None:
        b_bar = _sum_rows(pre_bar)
    if not need_b:
        b_bar = None
    return g_bar, x_bar, w_bar, b_bar


def _add(a, b):
    from .layers.modules import _binary_raw
    if a is None:
        return b
    if b is None:
        return a
    return _binary_raw(_ffi.MP_ADD, a, b)


class DenseAdjoint(torch.autograd.Function):
    """Dense's backward (dx, dW, db) as an op of (dy, x, W, b), for a backward in grad mode.

    ``pre = x W + b`` is not on the tape (the forward kernel computed it), so the reverse carries it by hand.  With
    upstreams hx, hW, hb on dx, dW, db: h_gp = hx W + x hW + hb (on gp = dy * act'(pre)); then csrc/mp_backward2.hip gives
    dy_bar = h_gp act'(pre) and pre_bar = h_gp dy act''(pre), and
    x_bar = gp hW^T + pre_bar W^T,  W_bar = hx^T gp + x^T pre_bar,  b_bar = sum_rows pre_bar."""

    @staticmethod
    def forward(ctx, g, x, kernel, bias, pre, act, alpha, want_x, want_w, want_b):
        ctx.set_materialize_grads(False)   # an output nobody uses (dW, db in the force pass) brings no upstream
        gc = g.contiguous()
        gx, gw, gb, gp = _affine_backward(_dense_ops(), gc, x, kernel, pre, act, alpha, want_x, want_w, want_b)
        ctx.g, ctx.x, ctx.kernel, ctx.pre, ctx.gp, ctx.act, ctx.alpha = gc, x, kernel, pre, gp, act, alpha
        return gx, gw, gb

    @staticmethod
    @once_differentiable
    def backward(ctx, hx, hw, hb):
        bars = _affine_adjoint_backward(_dense_ops(), ctx, hx, hw, hb)
        return (None,) * 10 if bars is None else bars + (None,) * 6


class Embedding(torch.autograd.Function):
    """Keras Embedding on float node numbers; backward = table gradient (``mp_embedding_grad_f32``)."""

    @staticmethod
    def forward(ctx, numbers, table):
        vocab, dim = int(table.shape[0]), int(table.shape[1])
        n = numbers.numel()
        out = torch.empty(tuple(numbers.shape) + (dim,), dtype=torch.float32, device=numbers.device)
        _ffi.call("mp_embedding_f32", _ffi.ptr(table), vocab, dim, _ffi.ptr(numbers), n, _ffi.ptr(out), None,
                  _ffi.stream())
        ctx.numbers, ctx.vocab, ctx.dim = numbers, vocab, dim
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        gc = g.contiguous()
        n = ctx.numbers.numel()
        nbytes = _ffi.workspace_bytes("mp_embedding_grad_ws_bytes", n, ctx.vocab)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=gc.device)
        out = torch.empty((ctx.vocab, ctx.dim), dtype=torch.float32, device=gc.device)
        _ffi.call("mp_embedding_grad_f32", _ffi.ptr(ctx.numbers), n, _ffi.ptr(gc), ctx.vocab, ctx.dim, _ffi.ptr(ws),
                  nbytes, _ffi.ptr(out), _ffi.stream())
        return None, out


class Softmax(torch.autograd.Function):
    """Row softmax on the last axis; backward from the saved output (``mp_softmax_rows_grad_f32``)."""

    @staticmethod
    def forward(ctx, x):
        xc = x.contiguous()
        c = int(xc.shape[-1])
        out = torch.empty_like(xc)
        _ffi.call("mp_softmax_rows_f32", _ffi.ptr(xc), xc.numel() // max(c, 1), c, _ffi.ptr(out), _ffi.stream())
        ctx.y = out
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        gc = g.contiguous()
        c = int(gc.shape[-1])
        out = torch.empty_like(gc)
        _ffi.call("mp_softmax_rows_grad_f32", _ffi.ptr(ctx.y), _ffi.ptr(gc), gc.numel() // max(c, 1), c, _ffi.ptr(out),
                  _ffi.stream())
        return out


class Activation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, act_code, alpha):
        xc = x.contiguous()
        ctx.x, ctx.x_in, ctx.act, ctx.alpha = xc, x, act_code, alpha
        out = torch.empty_like(xc)
        _ffi.call("mp_activation_f32", act_code, float(alpha), _ffi.ptr(xc), xc.numel(), _ffi.ptr(out), _ffi.stream())
        return out

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():
            return ActivationAdjoint.apply(ctx.x_in, g, ctx.act, ctx.alpha).view(ctx.x.shape), None, None
        return _activation_grad(ctx.x, g.contiguous(), ctx.act, ctx.alpha), None, None


def _activation_grad(xc, gc, act, alpha):
    out = torch.empty_like(gc)
    _ffi.call("mp_activation_grad_f32", act, float(alpha), _ffi.ptr(xc), _ffi.ptr(gc), gc.numel(), _ffi.ptr(out),
              _ffi.stream())
    return out


class ActivationAdjoint(torch.autograd.Function):
    """g * act'(x) as an op of (x, g); reverse: x_bar = h g act''(x), g_bar = h act'(x) (mp_activation_grad2_f32)."""

    @staticmethod
    def forward(ctx, x, g, act, alpha):
        xc, gc = x.contiguous(), g.contiguous()
        ctx.xc, ctx.gc, ctx.act, ctx.alpha = xc, gc, act, alpha
        return _activation_grad(xc, gc, act, alpha)

    @staticmethod
    @once_differentiable
    def backward(ctx, h):
        hc = h.contiguous()
        x_bar = torch.empty_like(hc) if ctx.needs_input_grad[0] else None
        g_bar = torch.empty_like(hc) if ctx.needs_input_grad[1] else None
        _ffi.call("mp_activation_grad2_f32", ctx.act, float(ctx.alpha), _ffi.ptr(ctx.xc), _ffi.ptr(ctx.gc), _ffi.ptr(hc),
                  _ffi.ptr(x_bar), _ffi.ptr(g_bar), hc.numel(), _ffi.stream())
        return x_bar, g_bar, None, None


def _unbroadcast(g, shape):
    """Sum ``g`` over the axes that were broadcast from ``shape`` (middle and / or last axis of the 3-D view, or the
    rows of a 2-D operand of one row)."""
    if tuple(g.shape) == tuple(shape):
        return g
    if g.dim() == 2 and len(shape) == 2 and int(shape[0]) == 1 and int(shape[1]) == int(g.shape[1]):
        return _sum_rows(g.contiguous()).reshape(shape)   # one row against all rows (INorp's c (N, 1) x b2 (1, H2))
    if g.dim() != len(shape) or int(g.shape[0]) != int(shape[0]):
        raise NotImplementedError("gradient of a row-broadcast operand is outside the force path")
    r = int(g.shape[0])
    cur = g.contiguous()
    last_b = int(shape[-1]) == 1 and int(g.shape[-1]) != 1
    mid_g = 1
    for d in g.shape[1:-1]:
        mid_g *= int(d)
    mid_s = 1
    for d in shape[1:-1]:
        mid_s *= int(d)
    mid_b = g.dim() > 2 and mid_s == 1 and mid_g != 1
    d2 = int(cur.shape[-1])
    if last_b:
        out = torch.empty((r, mid_g), dtype=torch.float32, device=g.device)
        _ffi.call("mp_sum_axis_f32", _ffi.ptr(cur), r, mid_g, d2, 2, _ffi.ptr(out), _ffi.stream())
        cur, d2 = out, 1
    if mid_b:
        src = cur.view(r, mid_g, d2)
        out = torch.empty((r, d2), dtype=torch.float32, device=g.device)
        _ffi.call("mp_sum_axis_f32", _ffi.ptr(src), r, mid_g, d2, 1, _ffi.ptr(out), _ffi.stream())
        cur = out
    return cur.reshape(shape)


class Binary(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, op):
        from .layers.modules import _binary_raw
        ctx.op, ctx.sa, ctx.sb = op, tuple(a.shape), tuple(b.shape)
        ctx.a = a if (op == _ffi.MP_MUL and b.requires_grad) else None
        ctx.b = b if (op == _ffi.MP_MUL and a.requires_grad) else None
        ctx.ga, ctx.gb = a.requires_grad, b.requires_grad
        return _binary_raw(op, a, b)

    @staticmethod
    def backward(ctx, g):
        from .layers.modules import _binary_raw
        gc = g.contiguous()
        ga = gb = None
        if torch.is_grad_enabled():
            return _binary_backward_differentiable(ctx, gc)
        if ctx.ga:
            ga = gc if ctx.op != _ffi.MP_MUL else _binary_raw(_ffi.MP_MUL, gc, ctx.b)
            ga = _unbroadcast(ga, ctx.sa)
        if ctx.gb:
            if ctx.op == _ffi.MP_MUL:
                gb = _binary_raw(_ffi.MP_MUL, gc, ctx.a)
            elif ctx.op == _ffi.MP_SUB:
                gb = torch.zeros_like(gc)
                gb = _binary_raw(_ffi.MP_SUB, gb, gc)
            else:
                gb = gc
            gb = _unbroadcast(gb, ctx.sb)
        return ga, gb, None


def _binary_backward_differentiable(ctx, gc):
    """Binary's backward on Binary itself (add / sub / mul without broadcasting), so that it is differentiable again."""
    from .layers.modules import binary_values
    if ctx.sa != ctx.sb:
        raise NotImplementedError("second derivative of a broadcasting elementwise op is not implemented")
    ga = gb = None
    if ctx.ga:
        ga = gc if ctx.op != _ffi.MP_MUL else binary_values(_ffi.MP_MUL, gc, ctx.b)
    if ctx.gb:
        if ctx.op == _ffi.MP_MUL:
            gb = binary_values(_ffi.MP_MUL, gc, ctx.a)
        elif ctx.op == _ffi.MP_SUB:
            gb = binary_values(_ffi.MP_SUB, torch.zeros_like(gc), gc)
        else:
            gb = gc
    return ga, gb, None


class ConcatLast(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *values):
        from .layers.modules import _concat_last_raw
        ctx.widths = [int(v.shape[-1]) for v in values]
        return _concat_last_raw(list(values))

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():     # a force pass through LazyConcatenate (HDNNP2nd): the reverse is recorded too
            return SplitWidths.apply(g, tuple(ctx.widths))
        return tuple(_split_widths(g, ctx.widths))


def _split_widths(g, widths):
    """ConcatLast's reverse: the column blocks of ``g`` as contiguous tensors."""
    gc = g.contiguous()
    total = int(gc.shape[-1])
    rows = gc.numel() // max(total, 1)
    outs, off = [], 0
    for w in widths:
        o = torch.empty(tuple(gc.shape[:-1]) + (w,), dtype=gc.dtype, device=gc.device)
        _ffi.call("mp_copy_cols_f32", _ffi.ptr(gc), total, off, _ffi.ptr(o), w, 0, rows, w, _ffi.stream())
        outs.append(o)
        off += w
    return outs


class SplitWidths(torch.autograd.Function):
    """ConcatLast's backward as a differentiable op of ``g``; its own backward is the concatenation again."""

    @staticmethod
    def forward(ctx, g, widths):
        return tuple(_split_widths(g, widths))

    @staticmethod
    def backward(ctx, *hs):
        return ConcatLast.apply(*[h.contiguous() for h in hs]), None


class SplitLast(torch.autograd.Function):
    @staticmethod
    def forward(ctx, value, num):
        from .layers.modules import _split_last_raw
        return tuple(_split_last_raw(value, num))

    @staticmethod
    def backward(ctx, *gs):
        if torch.is_grad_enabled():     # the concatenation is differentiable itself
            return ConcatLast.apply(*[g.contiguous() for g in gs]), None
        from .layers.modules import _concat_last_raw
        return _concat_last_raw([g.contiguous() for g in gs]), None


class EuclideanNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, r, d, c, flags, out_shape):
        xc = x.contiguous()
        ctx.x, ctx.x_in, ctx.rdc, ctx.flags = xc, x, (r, d, c), flags
        out = torch.empty(out_shape, dtype=torch.float32, device=x.device)
        _ffi.call("mp_euclidean_norm_f32", _ffi.ptr(xc), r, d, c, flags, _ffi.ptr(out), _ffi.stream())
        return out

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():
            if ctx.flags & (1 | 8):
                raise NotImplementedError("second derivative of the inverted / squared norm is not implemented")
            return EuclideanNormAdjoint.apply(ctx.x_in, g, ctx.rdc, ctx.flags), None, None, None, None, None
        return _euclidean_norm_grad(ctx.x, g.contiguous(), ctx.rdc, ctx.flags), None, None, None, None, None


def _euclidean_norm_grad(xc, gc, rdc, flags):
    r, d, c = rdc
    gx = torch.empty_like(xc)
    _ffi.call("mp_euclidean_norm_grad_f32", _ffi.ptr(xc), _ffi.ptr(gc), r, d, c, flags, _ffi.ptr(gx), _ffi.stream())
    return gx


class EuclideanNormAdjoint(torch.autograd.Function):
    """gx = g x / |x| as an op of (x, g) for the plain norm; reverse on mp_euclidean_norm_grad2_f32."""

    @staticmethod
    def forward(ctx, x, g, rdc, flags):
        xc, gc = x.contiguous(), g.contiguous()
        ctx.xc, ctx.gc, ctx.rdc, ctx.flags = xc, gc, rdc, flags
        return _euclidean_norm_grad(xc, gc, rdc, flags)

    @staticmethod
    @once_differentiable
    def backward(ctx, h):
        r, d, c = ctx.rdc
        hc = h.contiguous()
        x_bar = torch.empty_like(ctx.xc) if ctx.needs_input_grad[0] else None
        g_bar = torch.empty_like(ctx.gc) if ctx.needs_input_grad[1] else None
        _ffi.call("mp_euclidean_norm_grad2_f32", _ffi.ptr(ctx.xc), _ffi.ptr(ctx.gc), _ffi.ptr(hc), r, d, c, ctx.flags,
                  _ffi.ptr(x_bar), _ffi.ptr(g_bar), _ffi.stream())
        return x_bar, g_bar, None, None


class ScalarProduct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, axis):
        ac, bc = a.contiguous(), b.contiguous()
        ctx.a, ctx.b, ctx.axis = ac, bc, axis
        shape = list(ac.shape)
        r = 1
        for s in shape[:axis]:
            r *= int(s)
        c = 1
        for s in shape[axis + 1:]:
            c *= int(s)
        out = torch.empty(shape[:axis] + shape[axis + 1:], dtype=torch.float32, device=a.device)
        _ffi.call("mp_scalar_product_f32", _ffi.ptr(ac), _ffi.ptr(bc), r, int(shape[axis]), c, _ffi.ptr(out),
                  _ffi.stream())
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        from .layers.modules import _binary_raw
        ge = g.contiguous().unsqueeze(ctx.axis)
        return _binary_raw(_ffi.MP_MUL, ge, ctx.b), _binary_raw(_ffi.MP_MUL, ge, ctx.a), None


class BesselBasis(torch.autograd.Function):
    @staticmethod
    def forward(ctx, d, freq, num_radial, cutoff, exponent):
        dc = d.contiguous()
        ctx.d, ctx.freq, ctx.args = dc, freq, (num_radial, cutoff, exponent)
        out = torch.empty(tuple(dc.shape[:-1]) + (num_radial,), dtype=torch.float32, device=d.device)
        _ffi.call("mp_bessel_basis_f32", _ffi.ptr(dc), dc.numel(), _ffi.ptr(freq), num_radial, float(cutoff),
                  int(exponent), _ffi.ptr(out), _ffi.stream())
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        num_radial, cutoff, exponent = ctx.args
        gd = torch.empty_like(ctx.d)
        _ffi.call("mp_bessel_basis_grad_f32", _ffi.ptr(ctx.d), ctx.d.numel(), _ffi.ptr(ctx.freq), num_radial,
                  float(cutoff), int(exponent), _ffi.ptr(g.contiguous()), _ffi.ptr(gd), _ffi.stream())
        return gd, None, None, None, None


class GaussBasis(torch.autograd.Function):
    @staticmethod
    def forward(ctx, d, bins, distance, sigma, offset):
        dc = d.contiguous()
        ctx.d, ctx.d_in, ctx.args = dc, d, (bins, distance, sigma, offset)
        out = torch.empty(tuple(dc.shape[:-1]) + (bins,), dtype=torch.float32, device=d.device)
        _ffi.call("mp_gauss_basis_f32", _ffi.ptr(dc), dc.numel(), bins, distance, sigma, offset, _ffi.ptr(out),
                  _ffi.stream())
        return out

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():
            return GaussBasisAdjoint.apply(ctx.d_in, g, ctx.args), None, None, None, None
        return _gauss_basis_grad(ctx.d, g.contiguous(), ctx.args), None, None, None, None


def _gauss_basis_grad(dc, gc, args):
    bins, distance, sigma, offset = args
    gd = torch.empty_like(dc)
    _ffi.call("mp_gauss_basis_grad_f32", _ffi.ptr(dc), dc.numel(), bins, distance, sigma, offset, _ffi.ptr(gc),
              _ffi.ptr(gd), _ffi.stream())
    return gd


class GaussBasisAdjoint(torch.autograd.Function):
    """gd = sum_k g_k phi_k'(d) as an op of (d, g); reverse on mp_gauss_basis_grad2_f32."""

    @staticmethod
    def forward(ctx, d, g, args):
        dc, gc = d.contiguous(), g.contiguous()
        ctx.dc, ctx.gc, ctx.args = dc, gc, args
        return _gauss_basis_grad(dc, gc, args)

    @staticmethod
    @once_differentiable
    def backward(ctx, h):
        bins, distance, sigma, offset = ctx.args
        hc = h.contiguous()
        d_bar = torch.empty_like(ctx.dc) if ctx.needs_input_grad[0] else None
        g_bar = torch.empty_like(ctx.gc) if ctx.needs_input_grad[1] else None
        _ffi.call("mp_gauss_basis_grad2_f32", _ffi.ptr(ctx.dc), ctx.dc.numel(), bins, distance, sigma, offset,
                  _ffi.ptr(ctx.gc), _ffi.ptr(hc), _ffi.ptr(d_bar), _ffi.ptr(g_bar), _ffi.stream())
        return d_bar, g_bar, None


class CosCutoff(torch.autograd.Function):
    @staticmethod
    def forward(ctx, d, cutoff):
        dc = d.contiguous()
        ctx.d, ctx.cutoff = dc, cutoff
        out = torch.empty_like(dc)
        _ffi.call("mp_cos_cutoff_f32", _ffi.ptr(dc), dc.numel(), float(cutoff), _ffi.ptr(out), _ffi.stream())
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        gd = torch.empty_like(ctx.d)
        _ffi.call("mp_cos_cutoff_grad_f32", _ffi.ptr(ctx.d), ctx.d.numel(), float(ctx.cutoff),
                  _ffi.ptr(g.contiguous()), _ffi.ptr(gd), _ffi.stream())
        return gd, None


class LatticeShift(torch.autograd.Function):
    """``pos + image @ lattice`` per edge (``mp_lattice_shift_f32``).  Linear in the position with unit slope: the reverse
    is the upstream gradient itself, so the rule is differentiable any number of times.  The lattice gets no gradient
    (``ShiftPeriodicLattice`` refuses one that requires grad: stress is not implemented)."""

    @staticmethod
    def forward(ctx, pos, image, lattice, edge_splits):
        from .layers.geom import _lattice_shift_raw
        return _lattice_shift_raw(pos, image, lattice, edge_splits)

    @staticmethod
    def backward(ctx, g):
        return g, None, None, None


class FracToReal(torch.autograd.Function):
    """``A f`` per row (``mp_frac_to_real_f32``; ``transposed``: ``A^T f``).  Linear in ``f``: the reverse is the same rule
    with the other flag, so it is differentiable any number of times.  The lattice gets no gradient
    (``FracToRealCoordinates`` refuses one that requires grad)."""

    @staticmethod
    def forward(ctx, frac, lattice, row_splits, transposed):
        from .layers.geom import _frac_to_real_raw
        ctx.lattice, ctx.row_splits, ctx.transposed = lattice, row_splits, transposed
        return _frac_to_real_raw(frac, lattice, row_splits, transposed)

    @staticmethod
    def backward(ctx, g):
        return FracToReal.apply(g.contiguous(), ctx.lattice, ctx.row_splits, not ctx.transposed), None, None, None


class BatchNormInfer(torch.autograd.Function):
    """Inference batch normalisation (``mp_batchnorm_infer_f32``) as a function of its input alone: the reverse is
    ``g * inv`` on the same entry point, linear in ``g``.  The four vectors are constants (no weight gradients)."""

    @staticmethod
    def forward(ctx, x, layer):
        ctx.layer = layer
        return layer._infer_raw(x, reverse=False)

    @staticmethod
    def backward(ctx, g):
        return BatchNormInferScale.apply(g, ctx.layer), None


class BatchNormInferScale(torch.autograd.Function):
    """``g * inv``: its own reverse."""

    @staticmethod
    def forward(ctx, g, layer):
        ctx.layer = layer
        return layer._infer_raw(g, reverse=True)

    @staticmethod
    def backward(ctx, h):
        return BatchNormInferScale.apply(h, ctx.layer), None


# ------------------------------------------------------------------------------------------------ HDNNP2nd
_coordinate_hessian_discarded = [False]


@contextlib.contextmanager
def coordinate_hessian_discarded():
    """Set by ``EnergyForceModel.train_on_batch`` around ``total.backward(inputs=weights)``: there the second derivative of
    the symmetry functions with respect to the coordinates would only reach the coordinate leaf, which the step
    discards, so the ACSF adjoint may skip it.  Everywhere else asking for it raises ``NotImplementedError``."""
    prev = _coordinate_hessian_discarded[0]
    _coordinate_hessian_discarded[0] = True
    try:
        yield
    finally:
        _coordinate_hessian_discarded[0] = prev


class ACSF(torch.autograd.Function):
    """ACSFG2 / ACSFG4 of coordinates (N, 3) -> (N, R*m) on csrc/mp_acsf.hip; ``spec`` (layers/conv/acsf_conv.py) holds
    the atomic numbers, index plan and tables.  Backward: ``mp_acsf_g*_grad_f32``; in grad mode ``ACSFAdjoint``."""

    @staticmethod
    def forward(ctx, xyz, spec):
        ctx.spec, ctx.xyz = spec, xyz
        return spec.forward(xyz)

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():
            return ACSFAdjoint.apply(ctx.xyz, g, ctx.spec), None
        return ctx.spec.grad(ctx.xyz.detach(), g), None


class ACSFAdjoint(torch.autograd.Function):
    """dx = sum_m g dG_m/dx as an op of (x, g).  It is linear in g: g_bar = dG/dx . h on the JVP kernels
    (``mp_acsf_g*_jvp_f32``).  x_bar, the second derivative of G with respect to the coordinates, is not implemented:
    asking for it raises, except under ``coordinate_hessian_discarded()``, where it is skipped."""

    @staticmethod
    def forward(ctx, xyz, g, spec):
        ctx.spec, ctx.xyz = spec, xyz.detach()
        return spec.grad(ctx.xyz, g)

    @staticmethod
    @once_differentiable
    def backward(ctx, h):
        if ctx.needs_input_grad[0] and not _coordinate_hessian_discarded[0]:
            raise NotImplementedError("the second derivative of the symmetry functions with respect to the coordinates "
                                      "(a Hessian through ACSFG2 / ACSFG4) is not implemented")
        g_bar = ctx.spec.jvp(ctx.xyz, h) if ctx.needs_input_grad[1] else None
        return None, g_bar, None


class RelationalDense(torch.autograd.Function):
    """y = act(x W[rel] + b) (mp_relational_dense_f32); backward gp = dy * act'(pre), dx = gp W[rel]^T,
    dW[q] = x_q^T gp_q, db = sum gp, each only when asked.  In grad mode the backward is ``RelationalDenseAdjoint``."""

    @staticmethod
    def forward(ctx, x, kernel, bias, rel, act_code, alpha):
        from .layers.relational import relational_dense_raw
        pre, y = relational_dense_raw(x, kernel, bias, rel, act_code, alpha, keep_pre=act_code != 0)
        ctx.kernel, ctx.bias, ctx.rel, ctx.act, ctx.alpha, ctx.pre = kernel, bias, rel, act_code, alpha, pre
        ctx.x = x if (ctx.needs_input_grad[1] or ctx.needs_input_grad[0]) else None
        return y

    @staticmethod
    def backward(ctx, g):
        want_x = ctx.needs_input_grad[0]
        want_w = ctx.needs_input_grad[1] and not _input_grads_only[0]
        want_b = ctx.needs_input_grad[2] and not _input_grads_only[0]
        if torch.is_grad_enabled():
            gx, gw, gb = RelationalDenseAdjoint.apply(g, ctx.x, ctx.kernel, ctx.bias, ctx.rel, ctx.pre, ctx.act,
                                                      ctx.alpha, want_x, want_w, want_b)
            return gx, gw, gb, None, None, None
        gx, gw, gb, _ = _affine_backward(_relational_ops(ctx.rel, int(ctx.kernel.shape[0])), g.contiguous(), ctx.x,
                                         ctx.kernel, ctx.pre, ctx.act, ctx.alpha, want_x, want_w, want_b)
        return gx, gw, gb, None, None, None


class RelationalDenseAdjoint(torch.autograd.Function):
    """RelationalDense's backward (dx, dW, db) as an op of (dy, x, W, b) - ``DenseAdjoint`` with the relational kernels:
    h_gp = hx W[rel] + x hW[rel] + hb; dy_bar = h_gp act'(pre), pre_bar = h_gp dy act''(pre);
    x_bar = gp hW[rel]^T + pre_bar W[rel]^T,  W_bar = wgrad(hx, gp) + wgrad(x, pre_bar),  b_bar = sum_rows pre_bar."""

    @staticmethod
    def forward(ctx, g, x, kernel, bias, rel, pre, act, alpha, want_x, want_w, want_b):
        ctx.set_materialize_grads(False)
        gc = g.contiguous()
        gx, gw, gb, gp = _affine_backward(_relational_ops(rel, int(kernel.shape[0])), gc, x, kernel, pre, act, alpha,
                                          want_x, want_w, want_b)
        ctx.g, ctx.x, ctx.kernel, ctx.rel, ctx.pre, ctx.gp, ctx.act, ctx.alpha = gc, x, kernel, rel, pre, gp, act, alpha
        return gx, gw, gb

    @staticmethod
    @once_differentiable
    def backward(ctx, hx, hw, hb):
        bars = _affine_adjoint_backward(_relational_ops(ctx.rel, int(ctx.kernel.shape[0])), ctx, hx, hw, hb)
        return (None,) * 11 if bars is None else bars + (None,) * 7


# ------------------------------------------------------------------------------------------------ HDNNP4th
class RaggedToPadded(torch.autograd.Function):
    """Ragged values (N, F) -> zero-padded (G, Nmax, F) (``mp_ragged_to_padded_f32``, the kernel of ``ChangeTensorType``),
    for an output that a loss reaches (HDNNP4th's padded charges).  Backward: the real rows of the upstream gradient,
    gathered by ``mp_gather_rows_f32``."""

    @staticmethod
    def forward(ctx, values, row_splits, splits_host):
        counts = splits_host[1:] - splits_host[:-1]
        g, nmax = int(counts.size), int(counts.max()) if counts.size else 0
        vals = values.contiguous()
        width = vals.numel() // max(int(vals.shape[0]), 1)
        padded = torch.empty((g, nmax) + tuple(vals.shape[1:]), dtype=torch.float32, device=vals.device)
        _ffi.call("mp_ragged_to_padded_f32", _ffi.ptr(vals), _ffi.ptr(row_splits), g, nmax, max(width, 1),
                  _ffi.ptr(padded), None, _ffi.stream())
        ctx.splits_host, ctx.nmax, ctx.width, ctx.shape = splits_host, nmax, max(width, 1), tuple(vals.shape)
        return padded

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        import numpy as np
        s = ctx.splits_host
        counts = s[1:] - s[:-1]
        n = int(s[-1])
        graph = np.repeat(np.arange(counts.size, dtype=np.int64), counts)
        rows = (graph * ctx.nmax + np.arange(n, dtype=np.int64) - s[:-1][graph]).astype(np.int32)
        idx = torch.from_numpy(rows).to(g.device)
        out = torch.empty(ctx.shape, dtype=torch.float32, device=g.device)
        if n:
            _ffi.call("mp_gather_rows_f32", _ffi.ptr(g.contiguous()), int(counts.size) * ctx.nmax, ctx.width,
                      _ffi.ptr(idx), n, 1, _ffi.int32_array([0]), _ffi.ptr(out), _ffi.stream())
        return out, None, None


class CentCharge(torch.autograd.Function):
    """CENT charges Q (N, 1) of electronegativities chi (N,) and coordinates (N, 3) on csrc/mp_cent.hip; ``spec``
    (layers/conv/hdnnp_conv.py) holds the atomic numbers, molecule splits, total charges and tables.  Backward:
    ``mp_cent_charge_grad_f32`` (chi_bar = w, x_bar), each only when asked.  It is first order only: a backward in grad
    mode - the ``create_graph`` pass of a force loss - raises ``NotImplementedError``."""

    @staticmethod
    def forward(ctx, chi, xyz, spec):
        q = spec.forward(chi, xyz)
        ctx.spec, ctx.xyz, ctx.q = spec, xyz.detach(), q.detach()
        return q

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():
            raise NotImplementedError("second derivative of the charge equilibration (CENTCharge: a force loss or a "
                                      "create_graph backward through the charge solve) is not implemented")
        chi_bar, x_bar = ctx.spec.grad(ctx.xyz, ctx.q, g, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return chi_bar, x_bar, None


class GaussElectrostatics(torch.autograd.Function):
    """Electrostatic energy (G, 1) of Gaussian charges q (N,) at coordinates (N, 3) over the range indices
    (``mp_gauss_energy_f32``).  Backward: ``mp_gauss_energy_grad_f32`` (q_bar, x_bar), each only when asked; first order
    only, like ``CentCharge``."""

    @staticmethod
    def forward(ctx, q, xyz, spec):
        ctx.spec, ctx.q, ctx.xyz = spec, q.detach(), xyz.detach()
        return spec.forward(q, xyz)

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():
            raise NotImplementedError("second derivative of the charge equilibration's electrostatic energy "
                                      "(ElectrostaticEnergyGaussCharge) is not implemented")
        q_bar, x_bar = ctx.spec.grad(ctx.q, ctx.xyz, g, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return q_bar, x_bar, None


# ---------------------------------------------------------------------------------------------------------- DimeNet++
# First-order rules of csrc/mp_dimenet.hip (layers/geom.py EdgeAngle / VectorAngle, layers/conv/dimenet_conv.py).
# The weights of the DimeNet++ layers stay frozen, so no weight gradients; a backward in grad mode (a create_graph
# pass, i.e. a force loss) raises NotImplementedError, as the CENT rules do.

def _first_order_only(what, model="DimeNet++"):
    if torch.is_grad_enabled():
        raise NotImplementedError("second derivative of %s (a force loss or a create_graph backward through %s) "
                                  "is not implemented" % (what, model))


class VectorAngle(torch.autograd.Function):
    """theta (T, 1) of two vector rows (``mp_vector_angle_f32``); backward ``mp_vector_angle_grad_f32``."""

    @staticmethod
    def forward(ctx, v1, v2):
        from .layers.geom import vector_angle_raw
        ctx.v1, ctx.v2 = v1.detach().contiguous(), v2.detach().contiguous()
        return vector_angle_raw(ctx.v1, ctx.v2)

    @staticmethod
    def backward(ctx, g):
        _first_order_only("VectorAngle")
        t = int(ctx.v1.shape[0])
        g1 = torch.empty_like(ctx.v1) if ctx.needs_input_grad[0] else None
        g2 = torch.empty_like(ctx.v2) if ctx.needs_input_grad[1] else None
        if t and (g1 is not None or g2 is not None):
            _ffi.call("mp_vector_angle_grad_f32", _ffi.ptr(ctx.v1), _ffi.ptr(ctx.v2), t, _ffi.ptr(g.contiguous()),
                      _ffi.ptr(g1), _ffi.ptr(g2), _ffi.stream())
        return g1, g2


class EdgeAngle(torch.autograd.Function):
    """theta (T, 1) between the edge vectors of every angle pair (``spec``: layers/geom.py ``EdgeAngleSpec``); backward
    v_bar (E, 3) added per edge over both angle columns' CSR (``mp_edge_angle_grad_f32``)."""

    @staticmethod
    def forward(ctx, v, spec):
        ctx.v, ctx.spec = v.detach().contiguous(), spec
        return spec.forward(ctx.v)

    @staticmethod
    def backward(ctx, g):
        _first_order_only("EdgeAngle")
        return ctx.spec.grad(ctx.v, g), None


class SphericalBasis(torch.autograd.Function):
    """sbf (T, L*R) of distances d (E, 1) and angles theta (T, 1) (``spec``: layers/conv/dimenet_conv.py
    ``SphericalBasisSpec``); backward d_bar (E, 1) and theta_bar (T, 1), each only when asked."""

    @staticmethod
    def forward(ctx, d, theta, spec):
        sbf, rbf_env = spec.forward(d, theta)
        ctx.d, ctx.theta, ctx.spec, ctx.rbf_env = d.detach().contiguous(), theta.detach().contiguous(), spec, rbf_env
        return sbf

    @staticmethod
    def backward(ctx, g):
        _first_order_only("SphericalBasisLayer")
        d_bar, theta_bar = ctx.spec.grad(ctx.d, ctx.theta, ctx.rbf_env, g, ctx.needs_input_grad[0],
                                         ctx.needs_input_grad[1])
        return d_bar, theta_bar, None


class DimeTriplet(torch.autograd.Function):
    """Fused triplet step of DimNetInteractionPPBlock, out (E, 64) of xdown (E, 64) and sbf (T, L*R) (``spec``:
    layers/conv/dimenet_conv.py ``TripletSpec``, frozen W_sbf1 / W_sbf2); backward xdown_bar and sbf_bar."""

    @staticmethod
    def forward(ctx, xdown, sbf, spec):
        ctx.xdown, ctx.sbf, ctx.spec = xdown.detach().contiguous(), sbf.detach().contiguous(), spec
        return spec.forward(ctx.xdown, ctx.sbf)

    @staticmethod
    def backward(ctx, g):
        _first_order_only("the DimNetInteractionPPBlock triplet step")
        x_bar, s_bar = ctx.spec.grad(ctx.xdown, ctx.sbf, g, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return x_bar, s_bar, None


# --------------------------------------------------------------------------------------------------------------- EGNN
# First-order rules of csrc/mp_egnn.hip (layers/geom.py PositionEncodingBasisLayer, layers/conv/egnn_conv.py).  The fused
# edge step reads its weights in place and has no rule for them: the layer takes the layer sequence when one of them
# requires grad.  A backward in grad mode (a create_graph pass, i.e. a force loss) raises NotImplementedError.

class PositionEncoding(torch.autograd.Function):
    """[sin(x s) | cos(x s)] (M, 2K) of x (M, 1); backward x_bar = sum_k s_k (g_sin cos - g_cos sin)."""

    @staticmethod
    def forward(ctx, x, scales, interleave):
        from .layers.geom import position_encoding_raw
        ctx.x, ctx.scales, ctx.interleave = x.detach().contiguous(), scales, interleave
        return position_encoding_raw(ctx.x, scales, interleave)

    @staticmethod
    def backward(ctx, g):
        _first_order_only("PositionEncodingBasisLayer", "EGNN")
        m, k = int(ctx.x.shape[0]), int(ctx.scales.shape[0])
        x_bar = torch.empty_like(ctx.x)
        _ffi.call("mp_position_encoding_grad_f32", _ffi.ptr(ctx.x), m, _ffi.ptr(ctx.scales), k,
                  1 if ctx.interleave else 0, _ffi.ptr(g.contiguous()), _ffi.ptr(x_bar), _ffi.stream())
        return x_bar, None, None


class EgnnEdge(torch.autograd.Function):
    """Fused EGNN edge step, m_i (N, 128) of the node projections Pa, Pb (N, 128) and the norm output x (E, 1) (``spec``:
    layers/conv/egnn_conv.py ``EdgeStepSpec``, frozen weights); backward Pa_bar, Pb_bar and x_bar from the saved
    pre-activations."""

    @staticmethod
    def forward(ctx, pa, pb, x, spec):
        ctx.x, ctx.spec = x.detach().contiguous(), spec
        out, ctx.z1, ctx.z2 = spec.forward(pa.detach().contiguous(), pb.detach().contiguous(), ctx.x, save=True)
        return out

    @staticmethod
    def backward(ctx, g):
        _first_order_only("the fused EGNN edge step", "EGNN")
        a_bar, b_bar, x_bar = ctx.spec.grad(ctx.x, ctx.z1, ctx.z2, g, *ctx.needs_input_grad[:3])
        return a_bar, b_bar, x_bar, None


# ------------------------------------------------------------------------------------------------------------- MXMNet
# First-order rules of csrc/mp_mxmnet.hip (layers/conv/mxmnet_conv.py).  The weights of the MXMNet layers stay frozen, so
# there are no weight gradients; a backward in grad mode (a create_graph pass, i.e. a force loss) raises
# NotImplementedError.

class MxmEdge(torch.autograd.Function):
    """The multiplex edge message of MXMNet: ``out`` (N, W) (pool epilogue, ``base`` (N, W) or None added) or ``y``
    (E, W) (edge epilogue) of the node projections Pa, Pb (N, W) and the edge attributes a (E, Ka) (``spec``:
    layers/conv/mxmnet_conv.py ``EdgeMessageSpec``, frozen weights); backward Pa_bar, Pb_bar, a_bar from the saved
    pre-activation and gate, and g itself for ``base``."""

    @staticmethod
    def forward(ctx, pa, pb, a, base, spec):
        ctx.spec = spec
        out, ctx.z, ctx.l = spec.forward(pa.detach().contiguous(), pb.detach().contiguous(), a.detach().contiguous(),
                                         None if base is None else base.detach().contiguous(), save=True)
        return out

    @staticmethod
    def backward(ctx, g):
        _first_order_only("the fused MXMNet edge message", "MXMNet")
        g = g.contiguous()
        pa_bar, pb_bar, a_bar = ctx.spec.grad(ctx.z, ctx.l, g, *ctx.needs_input_grad[:3])
        return pa_bar, pb_bar, a_bar, (g if ctx.needs_input_grad[3] else None), None


class MxmTriplet(torch.autograd.Function):
    """The triplet pool of MXMLocalMP, out (E, W) of the edge messages x (E, W) and the basis rows s (T, W) (``spec``:
    layers/conv/mxmnet_conv.py ``TripletPoolSpec``); backward x_bar and s_bar, each only when asked."""

    @staticmethod
    def forward(ctx, x, s, spec):
        ctx.x, ctx.s, ctx.spec = x.detach().contiguous(), s.detach().contiguous(), spec
        return spec.forward(ctx.x, ctx.s)

    @staticmethod
    def backward(ctx, g):
        _first_order_only("the MXMLocalMP triplet pool", "MXMNet")
        x_bar, s_bar = ctx.spec.grad(ctx.x, ctx.s, g, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return x_bar, s_bar, None


# ---------------------------------------------------------------------------------------------------------------- GRU
class GRUCombine(torch.autograd.Function):
    """The GRUCell combine ``mp_gru_combine_f32`` of ``mx`` (R, 3U), ``mh`` (R, 3U) and the state ``h`` (R, U); backward
    ``mp_gru_combine_grad_f32``, which recomputes the gates from the three inputs.  The two products that form ``mx`` and
    ``mh`` are ``Dense`` rules of their own, so the cell's three weight gradients come from there.  First order."""

    @staticmethod
    def forward(ctx, mx, mh, h, act, rec_act):
        mx, mh, h = mx.contiguous(), mh.contiguous(), h.contiguous()
        ctx.act, ctx.rec_act = act, rec_act
        ctx.save_for_backward(mx, mh, h)
        out = torch.empty_like(h)
        _ffi.call("mp_gru_combine_f32", _ffi.ptr(mx), _ffi.ptr(mh), _ffi.ptr(h), int(h.shape[0]), int(h.shape[1]), act,
                  rec_act, _ffi.ptr(out), _ffi.stream())
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        mx, mh, h = ctx.saved_tensors
        want = ctx.needs_input_grad
        d_mx = torch.empty_like(mx) if want[0] else None
        d_mh = torch.empty_like(mh) if want[1] else None
        d_h = torch.empty_like(h) if want[2] else None
        if any(want[:3]):
            _ffi.call("mp_gru_combine_grad_f32", _ffi.ptr(mx), _ffi.ptr(mh), _ffi.ptr(h), _ffi.ptr(g.contiguous()),
                      int(h.shape[0]), int(h.shape[1]), ctx.act, ctx.rec_act, _ffi.ptr(d_mx), _ffi.ptr(d_mh),
                      _ffi.ptr(d_h), _ffi.stream())
        return d_mx, d_mh, d_h, None, None


# -------------------------------------------------------------------------------------------------------------- DMPNN
# First-order rule of the fused DMPNN round (layers/conv/dmpnn_conv.py DMPNNStep; csrc/mp_dmpnn.hip, csrc/mp_wgrad.hip).
# Unlike the EGNN edge step it returns the gradients of its weights, so the layer records it when the shared Dense trains.

class DirectedEdgeUpdate(torch.autograd.Function):
    """One fused DMPNN round, ``y = act2((R[send] - h[rev]) W + b + h0)`` with ``R`` the receiver sum of ``h``
    (``spec``: layers/conv/dmpnn_conv.py ``DirectedStepSpec``).  The forward is the fused route's two launches and saves
    ``R``, ``h`` and the output ``y``; the backward is csrc/mp_dmpnn.hip and the gathered-difference weight gradient of
    csrc/mp_wgrad.hip: ``h_bar``, ``h0_bar``, ``W_bar`` and ``b_bar``, each only when asked.  First order."""

    @staticmethod
    def forward(ctx, h, h0, kernel, bias, spec):
        hv = h.detach().contiguous()
        r, y = spec.forward(hv, h0.detach().contiguous(), kernel.detach(), None if bias is None else bias.detach())
        ctx.spec = spec
        ctx.save_for_backward(r, hv, y, kernel)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        r, hv, y, kernel = ctx.saved_tensors
        want_h, want_h0 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        want_w = ctx.needs_input_grad[2] and not _input_grads_only[0]
        want_b = ctx.needs_input_grad[3] and not _input_grads_only[0]
        h_bar, p, w_bar, b_bar = ctx.spec.grad(r, hv, y, kernel.detach(), g.contiguous(), want_h, want_w, want_b)
        return h_bar, (p if want_h0 else None), w_bar, b_bar, None


# -------------------------------------------------------------------------------------------------------------- INorp
# First-order rule of the folded INorp edge step (layers/conv/inorp_conv.py INorpEdgeStep; csrc/mp_inorp.hip).  The node
# products in front of it and the Dense behind it are ``Dense`` rules on row-block views of the first kernel, so torch's
# accumulation assembles the gradients of W1, b1, W2, b2 and of the nodes.

class InorpEdge(torch.autograd.Function):
    """``out[r] = pool over the edges of r of act(Pj[send] + Pi[recv] + edges Wc)`` (N, H1) (``spec``:
    layers/conv/inorp_conv.py ``EdgeStepSpec``).  The forward is the fused route's launch and saves nothing edge-sized:
    the backward recomputes the pre-activation (``mp_inorp_edge_grad_f32``) and returns ``Pj_bar``, ``Pi_bar``,
    ``edges_bar`` and ``Wc_bar``, each only when asked.  First order."""

    @staticmethod
    def forward(ctx, pj, pi, edges, wc, spec):
        pj, pi, edges, wc = pj.detach().contiguous(), pi.detach().contiguous(), edges.detach().contiguous(), wc.detach()
        ctx.spec = spec
        ctx.save_for_backward(pj, pi, edges, wc)
        return spec.forward(pj, pi, edges, wc)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        pj, pi, edges, wc = ctx.saved_tensors
        want = ctx.needs_input_grad
        want_wc = want[3] and not _input_grads_only[0]
        pj_bar, pi_bar, e_bar, wc_bar = ctx.spec.grad(pj, pi, edges, wc, g.contiguous(), want[0], want[2], want_wc)
        return pj_bar, (pi_bar if want[1] else None), e_bar, wc_bar, None


# -------------------------------------------------------------------------------------------------------------- MEGAN
# First-order rule of the fused importance readout (literature/MEGAN.py; csrc/mp_megan.hip): two launches forward, two
# in reverse, whatever the number of channels and attention layers.

MEGAN_READOUT_SIZES = {"max_channels": _ffi.MP_MEGAN_MAX_CHANNELS, "max_layers": _ffi.MP_MEGAN_MAX_LAYERS,
                       "max_width": _ffi.MP_MEGAN_MAX_WIDTH}


def megan_readout_values(x, z, plan, row_splits, g_rows, op, logits, want_p=False):
    """The two forward launches on detached, contiguous operands: ``(out (G, K W), ni (N, K), ei (M, K), p or None)``."""
    import ctypes
    n, w = int(x.shape[0]), int(x.shape[1])
    k = int(z.shape[1])
    m = plan.M
    if plan.K != 2 or plan.N != n:
        raise ValueError("the MEGAN readout takes (batch, [M], 2) indices over the %d nodes, got K=%d over %d nodes"
                         % (n, plan.K, plan.N))
    for t in logits:
        if t.numel() != m * k:
            raise ValueError("the MEGAN readout: attention logits of %d elements for %d edges and %d channels"
                             % (t.numel(), m, k))
    dev = x.device
    ei = torch.empty((m, k), dtype=torch.float32, device=dev)
    ni = torch.empty((n, k), dtype=torch.float32, device=dev)
    out = torch.empty((g_rows, k * w), dtype=torch.float32, device=dev)
    p = torch.empty((n, k), dtype=torch.float32, device=dev) if want_p else None
    ptr0, perm0, _ = plan.csr(0)
    ptr1, perm1, _ = plan.csr(1)
    group = (ctypes.c_void_p * len(logits))(*[_ffi.ptr(t).value for t in logits])
    _ffi.call("mp_megan_edge_importance_f32", len(logits), group, m, k, _ffi.ptr(ei), _ffi.stream())
    _ffi.call("mp_megan_readout_f32", _ffi.ptr(ei), m, k, _ffi.ptr(ptr0), _ffi.ptr(perm0), _ffi.ptr(ptr1),
              _ffi.ptr(perm1), _ffi.ptr(z), _ffi.ptr(x), n, w, _ffi.ptr(row_splits), g_rows, op, _ffi.ptr(p),
              _ffi.ptr(ni), _ffi.ptr(out), _ffi.stream())
    return out, ni, ei, p


class MeganReadout(torch.autograd.Function):
    """MEGAN's importance readout: from the node embeddings ``x`` (N, W), the linear output ``z`` (N, K) of the
    node-importance Dense chain and the ``L`` attention-logit tensors (M, K[, 1]) to ``(out (G, K W), node importances
    (N, K), edge importances (M, K))``.  The forward saves ``x``, ``z``, the pooled edge importances ``p`` and ``ei``;
    the backward is ``mp_megan_readout_grad_f32`` and ``mp_megan_edge_importance_grad_f32``: ``x_bar``, ``z_bar`` and
    one ``s_bar`` that is the gradient of every logit tensor.  First order."""

    @staticmethod
    def forward(ctx, x, z, plan, row_splits, g_rows, op, *logits):
        xc, zc = x.detach().contiguous(), z.detach().contiguous()
        lc = [t.detach().contiguous() for t in logits]
        out, ni, ei, p = megan_readout_values(xc, zc, plan, row_splits, g_rows, op, lc, want_p=True)
        ctx.plan, ctx.splits, ctx.g, ctx.op = plan, row_splits, g_rows, op
        ctx.logit_shapes = [tuple(t.shape) for t in logits]
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(xc, zc, p, ei)
        return out, ni, ei

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, g_ni, g_ei):
        x, z, p, ei = ctx.saved_tensors
        n, w = int(x.shape[0]), int(x.shape[1])
        m, k = int(ei.shape[0]), int(ei.shape[1])
        plan = ctx.plan
        dev = x.device
        if g_out is None:
            g_out = torch.zeros((ctx.g, k * w), dtype=torch.float32, device=dev)
        g_out = g_out.contiguous()
        g_ni = None if g_ni is None else g_ni.contiguous()
        g_ei = None if g_ei is None else g_ei.contiguous()
        x_bar = torch.empty_like(x)
        z_bar = torch.empty_like(z)
        q = torch.empty_like(z)
        _ffi.call("mp_megan_readout_grad_f32", _ffi.ptr(g_out), _ffi.ptr(g_ni), _ffi.ptr(x), _ffi.ptr(z), _ffi.ptr(p), n,
                  k, w, _ffi.ptr(ctx.splits), ctx.g, ctx.op, _ffi.ptr(x_bar), _ffi.ptr(z_bar), _ffi.ptr(q), _ffi.stream())
        s_bars = [None] * len(ctx.logit_shapes)
        if any(ctx.needs_input_grad[6:]):
            ptr0, _, _ = plan.csr(0)
            ptr1, _, _ = plan.csr(1)
            s_bar = torch.empty_like(ei)
            _ffi.call("mp_megan_edge_importance_grad_f32", _ffi.ptr(g_ei), _ffi.ptr(q), _ffi.ptr(ei), _ffi.ptr(plan.cols),
                      _ffi.ptr(ptr0), _ffi.ptr(ptr1), n, m, k, _ffi.ptr(s_bar), _ffi.stream())
            s_bars = [s_bar.view(shape) if want else None
                      for shape, want in zip(ctx.logit_shapes, ctx.needs_input_grad[6:])]
        return (x_bar if ctx.needs_input_grad[0] else None, z_bar if ctx.needs_input_grad[1] else None, None, None, None,
                None) + tuple(s_bars)
