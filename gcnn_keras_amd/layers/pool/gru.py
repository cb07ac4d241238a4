"""GRU readout over the node sequence of every graph: ``ks.layers.GRU(**pooling_gru)`` on a ragged ``(batch, [N], F)``
tensor as kgcnn/literature/CMPNN.py:157 calls it, returning the state after each graph's last node, ``(batch, units)``.

Constructor arguments and ``get_config()`` keys are ``ks.layers.GRU``'s; weights are in the Keras layout (as ``GRUUpdate``
holds them): ``kernel (F, 3u)``, ``recurrent_kernel (u, 3u)``, ``bias (2, 3u)`` (input / recurrent row), gates
``[z | r | h]``, ``reset_after=True``.  Two launches: the input product ``x W + b_in`` of all nodes on the matrix cores (``mp_dense_f32``) and
the whole recurrence in ``mp_gru_ragged_last_f32`` (csrc/mp_recurrent.hip) - the loop over the sequence runs inside the
kernel, a workgroup carries 16 graphs to the longest of them.  A graph without nodes returns the zero
state; the output has one row per graph, trailing empty graphs included.

Served: ``units`` a multiple of 4 up to 512, any input width, activations among the engine's codes; anything else that
changes the recurrence (``reset_after=False``, dropout, ``go_backwards``, ``return_sequences``, ``return_state``,
``stateful``, ``time_major``) raises ``NotImplementedError``.  Forward only: ``weight_gradients`` is off, so a call in grad
mode with trainable weights raises instead of leaving them off the tape.
"""
import torch

from ... import _ffi
from ..base import GraphBaseLayer
from ..modules import _dense_raw

MAX_UNITS = _ffi.MP_GRU_RAGGED_MAX_UNITS


class PoolingNodesGRU(GraphBaseLayer):

    weight_gradients = False   # forward only

    def __init__(self, units, activation="tanh", recurrent_activation="sigmoid", use_bias=True,
                 kernel_initializer="glorot_uniform", recurrent_initializer="orthogonal", bias_initializer="zeros",
                 kernel_regularizer=None, recurrent_regularizer=None, bias_regularizer=None, activity_regularizer=None,
                 kernel_constraint=None, recurrent_constraint=None, bias_constraint=None, dropout=0.0,
                 recurrent_dropout=0.0, return_sequences=False, return_state=False, go_backwards=False, stateful=False,
                 unroll=False, time_major=False, reset_after=True, **kwargs):
        super().__init__(**kwargs)
        if not reset_after:
            raise NotImplementedError("PoolingNodesGRU is built for the Keras default cell: reset_after=True")
        if dropout or recurrent_dropout:
            raise NotImplementedError("PoolingNodesGRU: dropout inside the recurrence is not built")
        if return_sequences or return_state or go_backwards or stateful or time_major:
            raise NotImplementedError("PoolingNodesGRU returns the state after each graph's last node: return_sequences, "
                                      "return_state, go_backwards, stateful and time_major are not built")
        self.units = int(units)
        if self.units < 4 or self.units % 4 or self.units > MAX_UNITS:
            raise NotImplementedError("PoolingNodesGRU serves units that are a multiple of 4, at most %d; got %d"
                                      % (MAX_UNITS, self.units))
        self._conf = {"units": units, "activation": activation, "recurrent_activation": recurrent_activation,
                      "use_bias": use_bias, "kernel_initializer": kernel_initializer,
                      "recurrent_initializer": recurrent_initializer, "bias_initializer": bias_initializer,
                      "kernel_regularizer": kernel_regularizer, "recurrent_regularizer": recurrent_regularizer,
                      "bias_regularizer": bias_regularizer, "activity_regularizer": activity_regularizer,
                      "kernel_constraint": kernel_constraint, "recurrent_constraint": recurrent_constraint,
                      "bias_constraint": bias_constraint, "dropout": dropout, "recurrent_dropout": recurrent_dropout,
                      "return_sequences": return_sequences, "return_state": return_state, "go_backwards": go_backwards,
                      "stateful": stateful, "unroll": unroll, "time_major": time_major, "reset_after": reset_after}
        for name in (activation, recurrent_activation):
            if (name.get("class_name", name.get("name")) if isinstance(name, dict) else name) not in _ffi.ACTIVATION_CODES:
                raise NotImplementedError("PoolingNodesGRU: activation %r is not among the engine's codes" % (name,))
        self._act = _ffi.activation_code(activation)
        self._rec = _ffi.activation_code(recurrent_activation)
        self.use_bias = use_bias
        self.kernel = self.recurrent_kernel = self.bias = None

    def build(self, input_shape):
        super().build(input_shape)
        in_dim, u = int(input_shape[-1]), self.units
        self.kernel = self.add_weight("gru_cell/kernel", (in_dim, 3 * u), self._conf["kernel_initializer"])
        self.recurrent_kernel = self.add_weight("gru_cell/recurrent_kernel", (u, 3 * u),
                                                self._conf["recurrent_initializer"])
        if self.use_bias:
            self.bias = self.add_weight("gru_cell/bias", (2, 3 * u), self._conf["bias_initializer"])

    def call(self, inputs, **kwargs):
        """inputs: nodes ``(batch, [N], F)`` -> ``(batch, units)``."""
        if kwargs.get("training"):
            raise NotImplementedError("PoolingNodesGRU is forward only")
        x = self.assert_ragged_input_rank(inputs)
        from ...autograd import needs_grad
        if needs_grad(x.values):
            raise NotImplementedError("%s (PoolingNodesGRU) has no reverse rule: its input requires grad; call it under "
                                      "torch.no_grad()" % self.name)
        vals = x.values.detach()
        _ffi.require_device(vals, x.row_splits)
        if vals.dtype != torch.float32 or vals.dim() != 2:
            raise ValueError("PoolingNodesGRU expects float32 nodes of shape (batch, [N], F)")
        n, g, u = int(vals.shape[0]), x.nrows(), self.units
        b_in = self.bias[0].detach() if self.bias is not None else None
        b_rec = self.bias[1].detach() if self.bias is not None else None
        mx = _dense_raw(vals, self.kernel.detach(), b_in, 0, 0.0) if n > 0 else None
        out = torch.empty((g, u), dtype=torch.float32, device=vals.device)
        _ffi.call("mp_gru_ragged_last_f32", _ffi.ptr(mx), n, _ffi.ptr(x.row_splits), g,
                  _ffi.ptr(self.recurrent_kernel.detach()), _ffi.ptr(b_rec), u, self._act, self._rec,
                  _ffi.ptr(out), _ffi.stream())
        return out

    def get_config(self):
        config = super().get_config()
        config.update(self._conf)
        return config
