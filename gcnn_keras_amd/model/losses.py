"""Keras losses for ``Model.compile`` (tf.keras.losses, reduction ``sum_over_batch_size``): the per-sample loss is taken
over the last axis, multiplied by the sample weight, and averaged over every sample - weight-zero samples included, as
Keras does.  This is torch plumbing on the model output ((G, 1) energies, (N, 7) class probabilities); the model's forward
and reverse pass are engine kernels."""
import numpy as np
import torch

from ..ragged import RaggedTensor

_EPS = 1e-7   # tf.keras.backend.epsilon()


def _values(t, like=None):
    if isinstance(t, RaggedTensor):
        return t.values
    if torch.is_tensor(t):
        return t
    dev = like.device if like is not None else None
    return torch.as_tensor(np.asarray(t, dtype=np.float32), device=dev)


def _reduce(per_sample, sample_weight):
    if sample_weight is not None:
        w = _values(sample_weight, per_sample).to(per_sample.dtype)
        per_sample = per_sample * w.reshape(per_sample.shape)
    return per_sample.mean()


def mean_absolute_error(y_pred, y_true, sample_weight=None):
    p = _values(y_pred)
    t = _values(y_true, p).to(p.dtype)
    return _reduce((p - t.reshape(p.shape)).abs().mean(dim=-1), sample_weight)


def mean_squared_error(y_pred, y_true, sample_weight=None):
    p = _values(y_pred)
    t = _values(y_true, p).to(p.dtype)
    return _reduce((p - t.reshape(p.shape)).square().mean(dim=-1), sample_weight)


def categorical_crossentropy(y_pred, y_true, sample_weight=None):
    """Keras ``categorical_crossentropy`` on probabilities: p / sum(p), clipped to [eps, 1 - eps], -sum y log p."""
    p = _values(y_pred)
    t = _values(y_true, p).to(p.dtype).reshape(p.shape)
    p = p / p.sum(dim=-1, keepdim=True)
    p = p.clamp(_EPS, 1.0 - _EPS)
    return _reduce(-(t * p.log()).sum(dim=-1), sample_weight)


_LOSSES = {"mean_absolute_error": mean_absolute_error, "mae": mean_absolute_error,
           "mean_squared_error": mean_squared_error, "mse": mean_squared_error,
           "categorical_crossentropy": categorical_crossentropy}


def get_loss(name):
    if callable(name):
        return name
    if not isinstance(name, str) or name not in _LOSSES:
        raise ValueError("Unknown loss %r (supported: %s)" % (name, ", ".join(sorted(_LOSSES))))
    return _LOSSES[name]
