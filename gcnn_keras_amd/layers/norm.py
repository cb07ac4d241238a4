"""Normalisation over the feature axis of a ragged tensor's values (mirror of kgcnn/layers/norm.py:8-221).

``GraphLayerNormalization`` is Keras ``LayerNormalization`` applied to ``.values``: the reference maps the user's axis
(counted on the ragged shape ``(batch, [N], F...)``, so it must not be 0) to ``axis - 1`` on the values
(norm.py:45-57).  The engine kernel normalises the last axis, which is the only use in the conv layers
(``GraphSageNodeLayer``, sage_conv.py:65); other axes are rejected.
``GraphBatchNormalization`` runs in inference mode, with the moving statistics (``mp_batchnorm_infer_f32``); batch
statistics and the moving-average update, training-time constructs, stay out of scope.
"""
import torch

from .. import _ffi
from ..autograd import needs_grad
from ..ragged import RaggedTensor
from .base import GraphBaseLayer


class GraphLayerNormalization(GraphBaseLayer):

    def __init__(self, axis=-1, epsilon=1e-3, center=True, scale=True, beta_initializer="zeros",
                 gamma_initializer="ones", beta_regularizer=None, gamma_regularizer=None, beta_constraint=None,
                 gamma_constraint=None, **kwargs):
        super().__init__(**kwargs)
        if isinstance(axis, (list, tuple)):
            if len(axis) != 1:
                raise NotImplementedError("the engine normalises one axis (the last)")
            axis = axis[0]
        if not isinstance(axis, int):
            raise TypeError("Expected an int or a list/tuple of ints for the argument 'axis', but received: %r" % axis)
        if axis == 0:
            raise ValueError("Positive axis for graph normalization must be > 0 or negative.")
        self.axis = axis
        self.epsilon, self.center, self.scale = float(epsilon), bool(center), bool(scale)
        self.beta_initializer, self.gamma_initializer = beta_initializer, gamma_initializer
        self.beta_regularizer, self.gamma_regularizer = beta_regularizer, gamma_regularizer
        self.beta_constraint, self.gamma_constraint = beta_constraint, gamma_constraint
        self.gamma = self.beta = None

    def build(self, input_shape):
        super().build(input_shape)
        n_dims = len(input_shape)
        axis = self.axis if self.axis >= 0 else n_dims + self.axis
        if axis < 1:
            raise ValueError("The (positive) axis must be > 0.")
        if axis != n_dims - 1:
            raise NotImplementedError("the engine normalises the last axis only")
        self.axis = axis                       # positive after build, like the reference (norm.py:89-90)
        width = int(input_shape[-1])
        if self.scale:                         # Keras creates gamma before beta
            self.gamma = self.add_weight("gamma", (width,), self.gamma_initializer)
        if self.center:
            self.beta = self.add_weight("beta", (width,), self.beta_initializer)

    def call(self, inputs, **kwargs):
        values = inputs.values if isinstance(inputs, RaggedTensor) else inputs
        _ffi.require_device(values)
        if needs_grad(values, self.gamma, self.beta):
            raise NotImplementedError("GraphLayerNormalization has no reverse pass on the engine yet")
        x = values.contiguous()
        width = int(x.shape[-1])
        rows = x.numel() // max(width, 1)
        out = torch.empty_like(x)
        _ffi.call("mp_layer_norm_f32", _ffi.ptr(x), rows, width, _ffi.ptr(self.gamma), _ffi.ptr(self.beta),
                  self.epsilon, _ffi.ptr(out), _ffi.stream())
        return inputs.with_values(out) if isinstance(inputs, RaggedTensor) else out

    def get_config(self):
        config = super().get_config()
        config.update({"axis": self.axis, "epsilon": self.epsilon, "center": self.center, "scale": self.scale,
                       "beta_initializer": self.beta_initializer, "gamma_initializer": self.gamma_initializer,
                       "beta_regularizer": self.beta_regularizer, "gamma_regularizer": self.gamma_regularizer,
                       "beta_constraint": self.beta_constraint, "gamma_constraint": self.gamma_constraint})
        return config


class GraphBatchNormalization(GraphBaseLayer):
    r"""Keras ``BatchNormalization`` on the values of a ragged tensor, **inference mode** (kgcnn/layers/norm.py:114-221):
    with the moving statistics, in Keras' order of operations,

    ``inv = (1 / sqrt(moving_variance + epsilon)) * gamma``,  ``y = x * inv + (beta - moving_mean * inv)``

    on ``mp_batchnorm_infer_f32``, which reads the four vectors where they are on every call.  Last axis only.  Weights
    in the order ``gamma, beta, moving_mean, moving_variance`` (``scale=False`` / ``center=False`` leave theirs out);
    Keras lists the two non-trainable statistics after every trainable weight of the MODEL, so a Keras weight list has
    to be reordered before ``set_weights``.  The reverse with respect to the input is ``g * inv``.  Batch statistics and
    the moving-average update are not built: ``call(..., training=True)`` raises, and the layer has no weight gradients,
    so training a batch-normalised model raises in ``layers/base.py`` rather than train against frozen statistics.

    ``get_config()`` has the reference's keys, which lack ``moving_variance_initializer`` and ``beta_regularizer``: the
    reference's key list misses a comma between the two (norm.py:181-183)."""

    def __init__(self, axis=-1, momentum=0.99, epsilon=0.001, center=True, scale=True, beta_initializer="zeros",
                 gamma_initializer="ones", moving_mean_initializer="zeros", moving_variance_initializer="ones",
                 beta_regularizer=None, gamma_regularizer=None, beta_constraint=None, gamma_constraint=None, **kwargs):
        super().__init__(**kwargs)
        if isinstance(axis, (list, tuple)):
            if any(x == 0 for x in axis):
                raise ValueError("Positive axis for graph normalization must be > 0 or negative.")
            if len(axis) != 1:
                raise NotImplementedError("the engine normalises one axis (the last)")
            axis = axis[0]
        if not isinstance(axis, int):
            raise TypeError("Expected an int or a list/tuple of ints for the argument 'axis', but received: %r" % axis)
        if axis == 0:
            raise ValueError("Positive axis for graph normalization must be > 0 or negative.")
        self.axis = axis
        self.momentum, self.epsilon = float(momentum), float(epsilon)
        self.center, self.scale = bool(center), bool(scale)
        self.beta_initializer, self.gamma_initializer = beta_initializer, gamma_initializer
        self.moving_mean_initializer = moving_mean_initializer
        self.moving_variance_initializer = moving_variance_initializer
        self.beta_regularizer, self.gamma_regularizer = beta_regularizer, gamma_regularizer
        self.beta_constraint, self.gamma_constraint = beta_constraint, gamma_constraint
        self.gamma = self.beta = self.moving_mean = self.moving_variance = None

    def build(self, input_shape):
        super().build(input_shape)
        n_dims = len(input_shape)
        axis = self.axis if self.axis >= 0 else n_dims + self.axis
        if axis < 1:
            raise ValueError("The (positive) axis must be > 0.")
        if axis != n_dims - 1:
            raise NotImplementedError("the engine normalises the last axis only")
        self.axis = axis                       # positive after build, like the reference (norm.py:201-202)
        width = int(input_shape[-1])
        if self.scale:                         # Keras' creation order: gamma, beta, moving_mean, moving_variance
            self.gamma = self.add_weight("gamma", (width,), self.gamma_initializer)
        if self.center:
            self.beta = self.add_weight("beta", (width,), self.beta_initializer)
        self.moving_mean = self.add_weight("moving_mean", (width,), self.moving_mean_initializer)
        self.moving_variance = self.add_weight("moving_variance", (width,), self.moving_variance_initializer)

    def _infer_raw(self, x, reverse=False):
        xc = x.contiguous()
        width = int(xc.shape[-1])
        if width != int(self.moving_variance.shape[0]):
            raise ValueError("%s was built for %d features, got %d" % (self.name, int(self.moving_variance.shape[0]), width))
        out = torch.empty_like(xc)
        _ffi.call("mp_batchnorm_infer_f32", _ffi.ptr(xc), xc.numel() // max(width, 1), width, _ffi.ptr(self.gamma),
                  None if reverse else _ffi.ptr(self.beta), None if reverse else _ffi.ptr(self.moving_mean),
                  _ffi.ptr(self.moving_variance), self.epsilon, _ffi.ptr(out), _ffi.stream())
        return out

    def call(self, inputs, training=False, **kwargs):
        if training:
            raise NotImplementedError("GraphBatchNormalization: batch statistics (training=True) are not implemented")
        values = inputs.values if isinstance(inputs, RaggedTensor) else inputs
        _ffi.require_device(values)
        if values.dtype != torch.float32:
            raise TypeError("GraphBatchNormalization expects float32 values, got %s" % values.dtype)
        if needs_grad(values):
            from ..autograd import BatchNormInfer
            out = BatchNormInfer.apply(values, self)
        else:
            out = self._infer_raw(values)
        return inputs.with_values(out) if isinstance(inputs, RaggedTensor) else out

    def get_config(self):
        config = super().get_config()
        config.update({"momentum": self.momentum, "epsilon": self.epsilon, "scale": self.scale, "center": self.center,
                       "beta_initializer": self.beta_initializer, "gamma_initializer": self.gamma_initializer,
                       "moving_mean_initializer": self.moving_mean_initializer,
                       "gamma_regularizer": self.gamma_regularizer, "beta_constraint": self.beta_constraint,
                       "gamma_constraint": self.gamma_constraint, "axis": self.axis})
        return config
