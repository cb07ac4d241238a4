"""``RelationalDense`` (mirror of kgcnn/layers/relational.py:10-260): a Dense layer with one kernel per relation,
``y = act(x W[rel] + b)``, on ``mp_relational_dense_f32`` (csrc/mp_relational.hip).  ``DecomposedRelationalDense`` adds
``num_bases`` / ``num_blocks``: the ``(num_relations, K, U)`` kernel is assembled on the device at call time
(``effective_kernel``)."""
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


def effective_kernel(kernel, lin_bases=None, num_blocks=None):
    """The ``(num_relations, K, U)`` kernel of a RelationalDense (kgcnn/layers/relational.py:204-217): the block-diagonal
    expansion of a ``(B, num_blocks, K / num_blocks, U / num_blocks)`` kernel (one strided copy per block into zeros), then
    ``lin_bases (num_relations, B) . kernel`` as a Dense on the ``(B, K U)`` view.  Device work only, no read-back: a
    captured HIP graph replays it; on a tape the gradients reach ``kernel`` and ``lin_bases`` through the copies and Dense."""
    from .modules import dense_values
    if num_blocks is not None:
        b, nb, k, u = (int(s) for s in kernel.shape)
        full = torch.zeros((b, nb * k, nb * u), dtype=kernel.dtype, device=kernel.device)
        for i in range(nb):
            full[:, i * k:(i + 1) * k, i * u:(i + 1) * u] = kernel[:, i]
        kernel = full
    if lin_bases is not None:
        b, k, u = (int(s) for s in kernel.shape)
        kernel = dense_values(lin_bases, kernel.reshape(b, k * u), None, "linear").view(int(lin_bases.shape[0]), k, u)
    return kernel


class RelationalDense(GraphBaseLayer):
    r"""``y_r = act(x_r W_{rel_r} + b)`` (kgcnn/layers/relational.py:10-260).  Inputs ``[features (batch, [N], F),
    relations (batch, [N])]``.  This class keeps what it has always done: one full kernel per relation, and
    ``NotImplementedError`` for ``num_bases`` / ``num_blocks`` (HDNNP's element MLPs and their tests rely on both).  The two
    decompositions are served by ``DecomposedRelationalDense`` below, the layer RGCN and GNNFilm build."""

    decompositions = False    # DecomposedRelationalDense: num_bases / num_blocks are served

    weight_gradients = True   # layers/base.py: no weight of this layer is left off the tape

    def __init__(self, units: int, num_relations: int, num_bases: int = None, num_blocks: int = None, activation=None,
                 use_bias: bool = True, kernel_initializer="glorot_uniform", bias_initializer="zeros",
                 kernel_regularizer=None, bias_regularizer=None, activity_regularizer=None, kernel_constraint=None,
                 bias_constraint=None, **kwargs):
        super().__init__(**kwargs)
        if (num_bases is not None or num_blocks is not None) and not self.decompositions:
            raise NotImplementedError("RelationalDense with num_bases / num_blocks is not implemented: use "
                                      "DecomposedRelationalDense")
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
        self.lin_bases = None
        self.bias = None

    def build(self, input_shape):
        super().build(input_shape)
        assert len(input_shape) == 2, "`RelationalDense` layer requires feature plus relation information."
        last = int(input_shape[0][-1])
        self._build_kernel(last)
        if self.use_bias:
            self.bias = self.add_weight("bias", (self.units,), self.bias_initializer)

    def _build_kernel(self, last):
        # every relation's kernel initialised on its own (relational.py:183-202): the fan is (in, units), not that of the
        # stacked (num_relations, in, units) tensor
        self.kernel = self.add_weight("kernel", (self.num_relations, last, self.units), self.kernel_initializer,
                                      fan=(last, self.units))

    def effective_kernel(self):
        """The ``(num_relations, K, U)`` kernel the layer applies."""
        return self.kernel

    def call(self, inputs, **kwargs):
        features, relations = self.assert_ragged_input_rank(list(inputs), ragged_rank=1)
        out = relational_dense_values(features.values, self.effective_kernel(), self.bias, relations.values,
                                      self.activation)
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


class DecomposedRelationalDense(RelationalDense):
    r"""``RelationalDense`` with the two regularisers of the RGCN paper, as the reference's layer has them
    (kgcnn/layers/relational.py:133-217).  ``num_bases``: the relations' kernels are combinations ``lin_bases . kernel`` of
    ``num_bases`` shared ones; ``num_blocks``: every kernel is block diagonal.  ``kernel`` is ``(num_bases or
    num_relations, [num_blocks,] K / num_blocks, U / num_blocks)``, ``lin_bases`` ``(num_relations, num_bases)``; weights in
    the reference's order ``kernel``, ``lin_bases``, ``bias``.  The ``(num_relations, K, U)`` kernel is assembled on the
    device at every call (``effective_kernel``).  Without either option the layer is a plain ``RelationalDense``."""

    decompositions = True

    def _build_kernel(self, last):
        multi = self.num_bases if self.num_bases is not None else self.num_relations
        if self.num_blocks is not None:
            assert last % self.num_blocks == 0 and self.units % self.num_blocks == 0, \
                "`num_blocks` must divide in- and output dimension."
            k, u = last // self.num_blocks, self.units // self.num_blocks
            # Keras takes a (num_blocks, k, u) slice as a convolution field: fans k * num_blocks and u * num_blocks
            self.kernel = self.add_weight("kernel", (multi, self.num_blocks, k, u), self.kernel_initializer,
                                          fan=(self.num_blocks * k, self.num_blocks * u))
        else:
            self.kernel = self.add_weight("kernel", (multi, last, self.units), self.kernel_initializer,
                                          fan=(last, self.units))
        if self.num_bases is not None:
            self.lin_bases = self.add_weight("lin_bases", (self.num_relations, self.num_bases), self.kernel_initializer)

    def effective_kernel(self):
        if self.num_bases is None and self.num_blocks is None:
            return self.kernel
        return effective_kernel(self.kernel, self.lin_bases, self.num_blocks)
