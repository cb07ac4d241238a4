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


def _real_rows(p, y_true):
    """A ragged per-atom target ``(B, [N], ...)`` against a padded prediction ``(B, Nmax, ...)`` whose element count
    differs from the target's (molecules of different sizes: the reshape below cannot pair them): the prediction's rows
    of the real atoms, by the target's row splits, and the target's values.  ``None`` for every other pair, which keeps
    the reshape (for molecules of one size it already pairs atom with atom)."""
    if not isinstance(y_true, RaggedTensor) or not torch.is_tensor(p):
        return None
    t = y_true.values
    if p.dim() != t.dim() + 1 or int(p.shape[0]) != y_true.nrows() or t.numel() == p.numel():
        return None
    splits = np.asarray(y_true.row_splits_host(), dtype=np.int64)
    counts = splits[1:] - splits[:-1]
    if tuple(p.shape[2:]) != tuple(t.shape[1:]) or (counts.size and int(counts.max()) > int(p.shape[1])):
        return None
    graph = np.repeat(np.arange(counts.size, dtype=np.int64), counts)
    local = np.arange(int(splits[-1]), dtype=np.int64) - splits[:-1][graph]
    rows = p[torch.from_numpy(graph).to(p.device), torch.from_numpy(local).to(p.device)]
    return rows, t.to(device=p.device, dtype=p.dtype)


def _per_sample(y_pred, y_true, sample_weight, term):
    p = _values(y_pred)
    real = _real_rows(p, y_true)
    if real is not None:
        # the mean runs over the real atoms of the batch, as the force loss does (flat_target)
        if sample_weight is not None:
            raise NotImplementedError("sample_weight with a ragged target against a padded prediction is not "
                                      "implemented")
        rows, t = real
        return term(rows - t).reshape(int(t.shape[0]), -1).mean(dim=-1).mean()
    t = _values(y_true, p).to(p.dtype)
    return _reduce(term(p - t.reshape(p.shape)).mean(dim=-1), sample_weight)


def mean_absolute_error(y_pred, y_true, sample_weight=None):
    return _per_sample(y_pred, y_true, sample_weight, torch.abs)


def mean_squared_error(y_pred, y_true, sample_weight=None):
    return _per_sample(y_pred, y_true, sample_weight, torch.square)


def categorical_crossentropy(y_pred, y_true, sample_weight=None):
    """Keras ``categorical_crossentropy`` on probabilities: p / sum(p), clipped to [eps, 1 - eps], -sum y log p."""
    p = _values(y_pred)
    t = _values(y_true, p).to(p.dtype).reshape(p.shape)
    p = p / p.sum(dim=-1, keepdim=True)
    p = p.clamp(_EPS, 1.0 - _EPS)
    return _reduce(-(t * p.log()).sum(dim=-1), sample_weight)


def binary_crossentropy(y_pred, y_true, sample_weight=None):
    """Keras ``binary_crossentropy`` on probabilities (``from_logits=False``, tf.keras.backend.binary_crossentropy): p
    clipped to [eps, 1 - eps], ``-(y log(p + eps) + (1 - y) log(1 - p + eps))``, mean over the last axis."""
    p = _values(y_pred)
    t = _values(y_true, p).to(p.dtype).reshape(p.shape)
    p = p.clamp(_EPS, 1.0 - _EPS)
    bce = t * torch.log(p + _EPS) + (1.0 - t) * torch.log(1.0 - p + _EPS)
    return _reduce(-bce.mean(dim=-1), sample_weight)


def flat_target(target, like, row_splits_host):
    """A per-atom target as the flat ``(N, ...)`` values of ``like`` (the model's flat output): a ``RaggedTensor`` gives
    its values, a flat array is taken as it is, a padded ``(B, Nmax, ...)`` array (one axis more than ``like``) is
    unpadded with the input's row splits, so that padding never enters a loss."""
    t = _values(target, like)
    if t.dim() == like.dim() + 1:
        splits = np.asarray(row_splits_host, dtype=np.int64)
        counts = splits[1:] - splits[:-1]
        if int(t.shape[0]) != counts.size or (counts.size and int(counts.max()) > int(t.shape[1])):
            raise ValueError("padded target of shape %s does not fit row splits with %d rows of at most %d atoms"
                             % (tuple(t.shape), counts.size, int(counts.max()) if counts.size else 0))
        graph = np.repeat(np.arange(counts.size, dtype=np.int64), counts)
        local = np.arange(int(splits[-1]), dtype=np.int64) - splits[:-1][graph]
        t = t[torch.from_numpy(graph).to(t.device), torch.from_numpy(local).to(t.device)]
    t = t.to(device=like.device, dtype=like.dtype)
    if t.numel() != like.numel():
        raise ValueError("target of shape %s does not match the output %s" % (tuple(t.shape), tuple(like.shape)))
    return t.reshape(like.shape)


_LOSSES = {"mean_absolute_error": mean_absolute_error, "mae": mean_absolute_error,
           "mean_squared_error": mean_squared_error, "mse": mean_squared_error,
           "categorical_crossentropy": categorical_crossentropy, "binary_crossentropy": binary_crossentropy}


def get_loss(name):
    if callable(name):
        return name
    if not isinstance(name, str) or name not in _LOSSES:
        raise ValueError("Unknown loss %r (supported: %s)" % (name, ", ".join(sorted(_LOSSES))))
    return _LOSSES[name]
