"""Host side of fit / predict / evaluate over a resident data set: the argument checks of ``mp_ragged_take``, the batch
rule ``batch_ids``, ``LinearLearningRateScheduler``, the batch-size-weighted ``History`` means and the no-CPU-fallback
guard of ``RaggedTensor.take``.  Nothing is launched (runs without a GPU)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from gcnn_keras_amd import _ffi
from gcnn_keras_amd.data.batching import batch_ids


def _desc(k=1, G=5, B=4, row_bytes=12, splits=0x1000, values=0x2000, flags=0x3000):
    """A descriptor whose pointers are never followed: every case here returns before a launch."""
    d = _ffi.TakeDesc()
    d.k, d.G, d.B, d.first, d.take, d.flags = k, G, B, 0, None, flags
    for i in range(min(max(k, 0), _ffi.MP_TAKE_MAX)):
        it = d.item[i]
        it.src_values, it.src_splits, it.row_bytes = values, splits, row_bytes
        it.dst_values, it.dst_splits, it.dst_rows = values, splits, 7
    return d


def _take(d):
    return _ffi.lib().mp_ragged_take(ctypes.byref(d), None)


def test_ragged_take_argument_errors():
    assert ctypes.sizeof(_ffi.TakeItem) == 48 and ctypes.sizeof(_ffi.TakeDesc) == 48 + 48 * _ffi.MP_TAKE_MAX
    assert _take(_desc(k=0)) == _ffi.MP_EINVAL
    with pytest.raises(ValueError):
        _ffi.check(_ffi.MP_EINVAL)
    assert b"mp_ragged_take" in _ffi.lib().mp_last_error()
    assert _take(_desc(k=_ffi.MP_TAKE_MAX + 1)) == _ffi.MP_EINVAL
    assert _take(_desc(splits=None)) == _ffi.MP_EINVAL
    for row_bytes in (6, 2, 0, 13):
        assert _take(_desc(row_bytes=row_bytes)) == _ffi.MP_EINVAL
    assert _take(_desc(flags=None)) == _ffi.MP_EINVAL
    assert _take(_desc(B=-1)) == _ffi.MP_EINVAL
    assert _ffi.lib().mp_ragged_take(None, None) == _ffi.MP_EINVAL
    # zero-sized problem: accepted without touching the device
    assert _take(_desc(B=0)) == _ffi.MP_OK
    assert _take(_desc(k=_ffi.MP_TAKE_MAX, B=0)) == _ffi.MP_OK


@pytest.mark.parametrize("G,b", [(23, 8), (16, 8), (7, 32), (1, 1), (37, 5)])
def test_batch_ids_rule(G, b):
    for shuffle in (False, True):
        ids = batch_ids(G, b, shuffle=shuffle, seed=3, epoch=2)
        assert len(ids) == math.ceil(G / b)
        assert [len(i) for i in ids[:-1]] == [b] * (len(ids) - 1) and len(ids[-1]) == G - b * (len(ids) - 1)   # tail kept
        assert all(i.dtype == np.int64 for i in ids)
        assert sorted(np.concatenate(ids).tolist()) == list(range(G))      # every id exactly once per epoch
    assert np.array_equal(np.concatenate(batch_ids(G, b, shuffle=False)), np.arange(G))
    perm = np.random.default_rng([3, 2]).permutation(G)                    # the stated expression
    got = batch_ids(G, b, shuffle=True, seed=3, epoch=2)
    assert all(np.array_equal(got[k], perm[k * b:(k + 1) * b]) for k in range(len(got)))
    again = batch_ids(G, b, shuffle=True, seed=3, epoch=2)
    assert all(np.array_equal(x, y) for x, y in zip(got, again))


def test_batch_ids_differ_between_epochs_and_seeds():
    e0 = np.concatenate(batch_ids(37, 8, shuffle=True, seed=3, epoch=0))
    e1 = np.concatenate(batch_ids(37, 8, shuffle=True, seed=3, epoch=1))
    s4 = np.concatenate(batch_ids(37, 8, shuffle=True, seed=4, epoch=0))
    assert not np.array_equal(e0, e1) and not np.array_equal(e0, s4)
    assert batch_ids(0, 8) == []
    with pytest.raises(ValueError):
        batch_ids(5, 0)


def _rule(start, stop, epo_min, epo, eps, epoch):
    if epoch < epo_min:
        return max(start, eps)
    return max(start - (start - stop) / (epo - epo_min) * (epoch - epo_min), eps)


def test_linear_learning_rate_scheduler():
    from gcnn_keras_amd.training.scheduler import LinearLearningRateScheduler
    start, stop, epo_min, epo, eps = 1e-3, 1e-5, 4, 20, 5e-6
    sched = LinearLearningRateScheduler(learning_rate_start=start, learning_rate_stop=stop, epo_min=epo_min, epo=epo,
                                        eps=eps)
    for epoch in (0, epo_min, (epo_min + epo) // 2, epo, epo + 5):
        assert sched.schedule_epoch_lr(epoch, 0.5) == pytest.approx(_rule(start, stop, epo_min, epo, eps, epoch), rel=1e-12)
    assert sched.schedule_epoch_lr(0) == start and sched.schedule_epoch_lr(epo_min) == start
    assert sched.schedule_epoch_lr((epo_min + epo) // 2) == pytest.approx(0.5 * (start + stop), rel=1e-12)
    assert sched.schedule_epoch_lr(epo) == pytest.approx(stop, rel=1e-12)
    assert sched.schedule_epoch_lr(epo + 5) == eps                          # the line is below eps there: the floor
    cfg = sched.get_config()
    assert cfg == {"verbose": 0, "learning_rate_start": start, "learning_rate_stop": stop, "epo": epo, "epo_min": epo_min,
                   "eps": eps}
    assert LinearLearningRateScheduler(**cfg).schedule_epoch_lr(9) == sched.schedule_epoch_lr(9)

    class Compiled:
        optimizer = None

    w = [torch.zeros(3, requires_grad=True), torch.zeros(2, requires_grad=True)]
    model = Compiled()
    model.optimizer = torch.optim.SGD([{"params": [w[0]]}, {"params": [w[1]], "lr": 0.5}], lr=0.1)
    sched.set_model(model)
    for epoch in (0, 12, 30):
        logs = {}
        sched.on_epoch_begin(epoch)
        sched.on_epoch_end(epoch, logs)
        want = _rule(start, stop, epo_min, epo, eps, epoch)
        assert [g["lr"] for g in model.optimizer.param_groups] == [pytest.approx(want, rel=1e-12)] * 2
        assert logs["lr"] == pytest.approx(want, rel=1e-12)
    model.optimizer = None
    with pytest.raises(ValueError):
        sched.on_epoch_begin(0)


class _Recorded:
    """A compiled model whose steps return recorded values: ``fit``'s bookkeeping without the engine."""

    def __init__(self, values):
        self.values, self.calls, self.optimizer = list(values), 0, object()

    def train_on_batch(self, x, y, sample_weight=None):
        self.calls += 1
        return self.values[self.calls - 1]


def test_history_means_are_batch_size_weighted(monkeypatch):
    from gcnn_keras_amd.model import loop
    sizes = []

    def fake_take(tensors, ids_device, ids_host, ids_device_i32=None, ragged_validate=False):
        sizes.append(len(ids_host))
        return list(tensors)

    monkeypatch.setattr(loop, "take_batch", fake_take)
    monkeypatch.setattr(loop, "_device_of", lambda x: "cpu")
    x, y = [torch.zeros(23, 2)], torch.zeros(23, 1)
    model = _Recorded([1.0, 2.0, 4.0, 3.0, 5.0, 6.0])
    stops = []

    class Stop(loop.Callback):
        def on_epoch_end(self, epoch, logs=None):
            stops.append((epoch, dict(logs)))

    hist = loop.fit(model, ["loss"], x, y, batch_size=8, epochs=2, shuffle=False, callbacks=[Stop()], seed=None)
    assert sizes == [8, 8, 7, 8, 8, 7] and model.calls == 6
    assert hist.history["loss"] == [pytest.approx((1.0 * 8 + 2.0 * 8 + 4.0 * 7) / 23, rel=1e-15),
                                    pytest.approx((3.0 * 8 + 5.0 * 8 + 6.0 * 7) / 23, rel=1e-15)]
    assert hist.history["loss"][0] != pytest.approx((1.0 + 2.0 + 4.0) / 3)   # not the plain mean over batches
    assert hist.epoch == [0, 1] and [e for e, _ in stops] == [0, 1]
    assert hist.params["batch_size"] == 8 and hist.params["steps"] == 3 and isinstance(hist.params["seed"], int)
    assert loop.weighted_mean([1.0, 2.0, 4.0], [8, 8, 7]) == hist.history["loss"][0]
    # three named outputs (the force model), and a callback that stops the training after the first epoch
    model = _Recorded([[3.0, 1.0, 2.0], [6.0, 2.0, 4.0], [9.0, 3.0, 6.0]] * 2)

    class StopNow(loop.Callback):
        def on_epoch_end(self, epoch, logs=None):
            self.model.stop_training = True

    hist = loop.fit(model, ["loss", "energy_loss", "force_loss"], x, [y, y], batch_size=8, epochs=2, shuffle=False,
                    callbacks=[StopNow()], seed=1)
    assert model.calls == 3 and hist.epoch == [0] and hist.params["seed"] == 1
    assert hist.history["energy_loss"] == [pytest.approx((1.0 * 8 + 2.0 * 8 + 3.0 * 7) / 23, rel=1e-15)]
    assert set(hist.history) == {"loss", "energy_loss", "force_loss"}


def test_take_on_cpu_tensors_raises():
    from gcnn_keras_amd.data.batching import take_batch
    from gcnn_keras_amd.ragged import RaggedTensor
    r = RaggedTensor(torch.zeros(5, 3), torch.tensor([0, 2, 5]))
    with pytest.raises(_ffi.EngineError):
        r.take([1, 0])
    with pytest.raises(_ffi.EngineError):
        take_batch([r, torch.zeros(2, 1)], None, np.arange(2))
    with pytest.raises(_ffi.EngineError):
        take_batch([torch.zeros(2, 1)], None, np.arange(2))
