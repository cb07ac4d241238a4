"""``RelationalDense`` (mirror of kgcnn/layers/relational.py:10-260 without ``num_bases`` / ``num_blocks``): a Dense layer
with one kernel per relation, ``y = act(x W[rel] + b)``, on ``mp_relational_dense_f32`` (csrc/mp_relational.hip)."""
import torch

from .. import _ffi
from .base import GraphBaseLayer
from .modules import _activation_name


def relational_dense_raw(x, kernel, bias, rel, act_code, alpha, keep_pre=False):
    """(pre, y): ``y = act(x W[rel] + b)`` with the pre-activation kept when ``keep_pre``."""
    nrel, k, u = (int(s) for s in kernel.shape)
    xc = x.contiguous()
    rows = xc.numel() // max(k, 1)
    y = torch.empty(tuple(x.shape[:-1]) + (u,), dtype=torch.float32, device=x.device)
    pre = torch.empty_like(y) if keep_pre else None
    _ffi.call("mp_relational_dense_f32", _ffi.ptr(xc), rows, k, _ffi.ptr(rel), nrel, _ffi.ptr(kernel), _ffi.ptr(bias),
              u, act_code, float(alpha), 0, None, _ffi.ptr(pre), _ffi.ptr(y), _ffi.stream())
    return pre, y


def relational_dense_t_raw(g, kernel, rel, act_code=0, alpha=0.0, pre=None):
    """``(g * act'(pre)) W[rel]^T`` (pre None: no factor) - the input gradient of a RelationalDense."""
    nrel, k, u = (int(s) for s in kernel.shape)
    gc = g.contiguous()
    rows = gc.numel() // max(u, 1)
    y = torch.empty(tuple(g.shape[:-1]) + (k,), dtype=torch.float32, device=g.device)
    _ffi.call("mp_relational_dense_f32", _ffi.ptr(gc), rows, k, _ffi.ptr(rel), nrel, _ffi.ptr(kernel), None, u,
              act_code, float(alpha), 1, _ffi.ptr(pre), None, _ffi.ptr(y), _ffi.stream())
    return y


def relational_wgrad(x, g, rel, nrel, with_kernel=True, with_bias=True):
    """``(dW (nrel, K, U), db (U))`` on ``mp_relational_dense_wgrad_f32``; either may be skipped (None)."""
    k, u = int(x.shape[-1]), int(g.shape[-1])
    xc, gc = x.contiguous(), g.contiguous()
    rows = gc.numel() // max(u, 1)
    dw = torch.empty((nrel, k, u), dtype=torch.float32, device=g.device) if with_kernel else None
    db = torch.empty((u,), dtype=torch.float32, device=g.device) if with_bias else None
    nbytes, ws = 0, None
    if with_kernel:
        nbytes = _ffi.workspace_bytes("mp_relational_dense_wgrad_ws_bytes", rows, nrel)
        ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=g.device)
    _ffi.call("mp_relational_dense_wgrad_f32", _ffi.ptr(xc), rows, k, _ffi.ptr(rel), nrel, _ffi.ptr(gc), u,
              _ffi.ptr(dw), _ffi.ptr(db), _ffi.ptr(ws), nbytes, _ffi.stream())
    return dw, db


def relational_dense_values(x, kernel, bias, rel, activation="linear", alpha=0.05):
    from ..autograd import RelationalDense as RelationalDenseFn, needs_grad
    _ffi.require_device(x, kernel, rel)
    if x.dtype != torch.float32:
        raise TypeError("RelationalDense expects float32 values, got %s" % x.dtype)
    if int(x.shape[-1]) != int(kernel.shape[1]):
        raise ValueError("RelationalDense kernel expects last dimension %d, got %d" % (int(kernel.shape[1]),
                                                                                      int(x.shape[-1])))
    relc = rel.contiguous() if rel.dtype == torch.int64 else rel.to(torch.int64).contiguous()
    if int(relc.numel()) != x.numel() // max(int(x.shape[-1]), 1):
        raise ValueError("RelationalDense needs one relation per row")
    code = _ffi.activation_code(_activation_name(activation))
    if needs_grad(x, kernel, bias):
        return RelationalDenseFn.apply(x, kernel, bias, relc, code, float(alpha))
    return relational_dense_raw(x, kernel, bias, relc, code, alpha)[1]


class RelationalDense(GraphBaseLayer):
    r"""``y_r = act(x_r W_{rel_r} + b)`` (kgcnn/layers/relational.py:10-260).  Inputs ``[features (batch, [N], F),
    relations (batch, [N])]``.  The basis and block-diagonal decompositions raise ``NotImplementedError``."""

    weight_gradients = True   # layers/base.py: no weight of this layer is left off the tape

    def __init__(self, units: int, num_relations: int, num_bases: int = None, num_blocks: int = None, activation=None,
                 use_bias: bool = True, kernel_initializer="glorot_uniform", bias_initializer="zeros",
                 kernel_regularizer=None, bias_regularizer=None, activity_regularizer=None, kernel_constraint=None,
                 bias_constraint=None, **kwargs):
        super().__init__(**kwargs)
        if num_bases is not None or num_blocks is not None:
            raise NotImplementedError("RelationalDense with num_bases / num_blocks is not implemented")
        self.units = int(units)
        self.num_relations = int(num_relations)
        self.num_bases, self.num_blocks = num_bases, num_blocks
        self.activation = _activation_name(activation)
        self.use_bias = use_bias
        self.kernel_initializer, self.bias_initializer = kernel_initializer, bias_initializer
        self.kernel_regularizer, self.bias_regularizer = kernel_regularizer, bias_regularizer
        self.activity_regularizer = activity_regularizer
        self.kernel_constraint, self.bias_constraint = kernel_constraint, bias_constraint
        self.kernel = None
        self.bias = None

    def build(self, input_shape):
        super().build(input_shape)
        assert len(input_shape) == 2, "`RelationalDense` layer requires feature plus relation information."
        last = int(input_shape[0][-1])
        # every relation's kernel initialised on its own (relational.py:183-202): the fan is (in, units), not that of the
        # stacked (num_relations, in, units) tensor
        self.kernel = self.add_weight("kernel", (self.num_relations, last, self.units), self.kernel_initializer,
                                      fan=(last, self.units))
        if self.use_bias:
            self.bias = self.add_weight("bias", (self.units,), self.bias_initializer)

    def call(self, inputs, **kwargs):
        features, relations = self.assert_ragged_input_rank(list(inputs), ragged_rank=1)
        out = relational_dense_values(features.values, self.kernel, self.bias, relations.values, self.activation)
        return features.with_values(out)

    def get_config(self):
        config = super().get_config()
        config.update({"units": self.units, "use_bias": self.use_bias, "num_relations": self.num_relations,
                       "num_bases": self.num_bases, "num_blocks": self.num_blocks,
                       "kernel_initializer": self.kernel_initializer, "bias_initializer": self.bias_initializer,
                       "kernel_regularizer": self.kernel_regularizer, "bias_regularizer": self.bias_regularizer,
                       "kernel_constraint": self.kernel_constraint, "bias_constraint": self.bias_constraint,
                       "activation": self.activation, "activity_regularizer": self.activity_regularizer})
        return config
