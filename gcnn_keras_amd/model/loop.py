"""The Keras loop around a per-batch model: ``fit``, ``predict(batch_size=...)`` and ``evaluate`` over a resident data set
(kgcnn/training/train_qm.py:159-186: ``model.fit(x_train, y_train, validation_data=..., batch_size=..., epochs=...,
shuffle=True, callbacks=[...])`` then ``model.predict(x, batch_size=...)``).

Shared by ``Model`` and ``EnergyForceModel``.  The data set is the list of device tensors that
``MemoryGraphList.tensor(...)`` returns; every batch is cut out of it on the GPU (``data.batching.take_batch``) on the
current stream, and takes whatever route ``model(inputs)`` takes for a batch it sees for the first time.  Host code
here is the loop, the callbacks and the bookkeeping of the loss values.
"""
import numpy as np
import torch

from ..data.batching import batch_ids, num_graphs, take_batch
from ..ragged import RaggedTensor


class Callback:
    """The part of ``ks.callbacks.Callback`` the fork's training scripts use."""

    model = None

    def set_model(self, model):
        self.model = model

    def on_train_begin(self, logs=None):
        pass

    def on_train_end(self, logs=None):
        pass

    def on_epoch_begin(self, epoch, logs=None):
        pass

    def on_epoch_end(self, epoch, logs=None):
        pass


class History(Callback):
    """``ks.callbacks.History``: ``epoch``, ``params`` and ``history`` (one list per logged name)."""

    def __init__(self):
        self.epoch, self.params, self.history = [], {}, {}

    def on_epoch_end(self, epoch, logs=None):
        self.epoch.append(epoch)
        for name, value in (logs or {}).items():
            self.history.setdefault(name, []).append(value)


def weighted_mean(values, counts):
    """Mean over batches weighted by graphs per batch (Keras' loss tracker): ``sum(v_i n_i) / sum(n_i)``."""
    total = 0.0
    for v, n in zip(values, counts):
        total += float(v) * int(n)
    return total / float(sum(int(n) for n in counts))


def _as_list(x):
    return list(x) if isinstance(x, (list, tuple)) else [x]


def resident(members, device):
    """Members of a data set on the device: ``RaggedTensor`` and device tensors as they are, host arrays uploaded once
    (floating point as float32, the engine's type); ``None`` stays."""
    out = []
    for t in members:
        if t is None or isinstance(t, RaggedTensor) or (torch.is_tensor(t) and t.is_cuda):
            out.append(t)
            continue
        a = t.numpy() if torch.is_tensor(t) else np.asarray(t)
        if a.dtype.kind == "f":
            a = a.astype(np.float32, copy=False)
        out.append(torch.from_numpy(np.ascontiguousarray(a)).to(device))
    return out


def _device_of(x):
    for t in _as_list(x):
        if isinstance(t, RaggedTensor):
            return t.values.device
        if torch.is_tensor(t) and t.is_cuda:
            return t.device
    from .. import _ffi
    raise _ffi.EngineError("the data set must be resident on the GPU (MemoryGraphList.tensor(...)); no CPU fallback")


class _Epoch:
    """The batches of one epoch: host id arrays by the batch rule, and (shuffled) their device copies uploaded once."""

    def __init__(self, G, batch_size, shuffle, seed, epoch, device):
        self.ids = batch_ids(G, batch_size, shuffle=shuffle, seed=seed, epoch=epoch)
        self.order = self.order32 = None
        if shuffle and G:
            self.order = torch.from_numpy(np.concatenate(self.ids)).to(device)
            self.order32 = self.order.to(torch.int32)
        self.batch_size = int(batch_size)

    def take(self, k, members):
        """Batch ``k`` of every member list in ``members`` (lists of tensors; ``None`` lists stay ``None``)."""
        ids = self.ids[k]
        a = k * self.batch_size
        dev = None if self.order is None else self.order[a:a + ids.shape[0]]
        dev32 = None if self.order32 is None else self.order32[a:a + ids.shape[0]]
        flat, spans = [], []
        for m in members:
            spans.append(None if m is None else (len(flat), len(flat) + len(m)))
            flat.extend(m or [])
        got = take_batch(flat, dev, ids, ids_device_i32=dev32)
        return [None if s is None else got[s[0]:s[1]] for s in spans]


def _like(structure, members):
    """``members`` (a list) in the form the caller passed ``structure``: a single tensor, a list or a tuple."""
    if structure is None:
        return None
    if isinstance(structure, (list, tuple)):
        return type(structure)(members)
    return members[0]


def _members(structure):
    return None if structure is None else _as_list(structure)


# ---- predict -----------------------------------------------------------------------------------------------------------
class _Dense:
    """One dense output leaf: ``(B, ...)`` per batch into one ``(G, ...)`` tensor allocated at the first batch.  A padded
    per-atom output ``(B, Nmax_b, ...)`` lands in a zero-filled ``(G, Nmax, ...)`` that widens when a later batch is."""

    def __init__(self, G):
        self.G, self.out = G, None

    def add(self, a, b, o):
        if self.out is None:
            make = torch.zeros if o.dim() >= 3 else torch.empty
            self.out = make((self.G,) + tuple(o.shape[1:]), dtype=o.dtype, device=o.device)
        if tuple(o.shape[1:]) == tuple(self.out.shape[1:]):
            self.out[a:b].copy_(o)
            return
        if o.dim() < 3 or tuple(o.shape[2:]) != tuple(self.out.shape[2:]):
            raise ValueError("batch outputs of shapes %s and %s cannot be assembled" % (tuple(o.shape),
                                                                                       tuple(self.out.shape)))
        if int(o.shape[1]) > int(self.out.shape[1]):
            wide = torch.zeros((self.G, int(o.shape[1])) + tuple(o.shape[2:]), dtype=o.dtype, device=o.device)
            wide[:a, :self.out.shape[1]].copy_(self.out[:a])
            self.out = wide
        self.out[a:b, :o.shape[1]].copy_(o)

    def result(self, x):
        return self.out


class _Ragged:
    """One ragged output leaf: values concatenated; the splits are those of the input with the same partition."""

    def __init__(self, G):
        self.values, self.lengths = [], []

    def add(self, a, b, o):
        s = o.row_splits_host()
        self.values.append(o.values)
        self.lengths.append(s[1:] - s[:-1])

    def result(self, x):
        splits = np.zeros(sum(len(n) for n in self.lengths) + 1, dtype=np.int64)
        np.cumsum(np.concatenate(self.lengths), out=splits[1:])
        values = torch.cat(self.values, dim=0)
        for t in x:
            if isinstance(t, RaggedTensor) and np.array_equal(t.row_splits_host(), splits):
                return t.with_values(values)
        out = RaggedTensor(values, torch.from_numpy(splits).to(values.device))
        out._splits_host = splits
        return out


class _Other:
    def __init__(self, G):
        self.value = None

    def add(self, a, b, o):
        self.value = o

    def result(self, x):
        return self.value


def _collector(o, G):
    if isinstance(o, dict):
        return {k: _collector(v, G) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return type(o)(_collector(v, G) for v in o)
    if isinstance(o, RaggedTensor):
        return _Ragged(G)
    if torch.is_tensor(o) and o.dim() >= 1:
        return _Dense(G)
    return _Other(G)


def _walk(col, o, fn):
    if isinstance(col, dict):
        return {k: _walk(c, None if o is None else o[k], fn) for k, c in col.items()}
    if isinstance(col, (list, tuple)):
        return type(col)(_walk(c, None if o is None else o[i], fn) for i, c in enumerate(col))
    return fn(col, o)


def predict(model, x, batch_size, kwargs):
    """``model.predict(x, batch_size)``: the data set in order, ``batch_size`` graphs per model call, the results assembled
    on the device into what one call over the whole data set returns (structure kept)."""
    xs = _as_list(x)
    G = num_graphs(xs)
    epoch = _Epoch(G, batch_size, False, 0, 0, _device_of(xs))
    col, a = None, 0
    for k, ids in enumerate(epoch.ids):
        xb, = epoch.take(k, [xs])
        out = model(_like(x, xb), **kwargs)
        if col is None:
            col = _collector(out, G)
        b = a + int(ids.shape[0])
        _walk(col, out, lambda c, o: c.add(a, b, o.detach() if torch.is_tensor(o) else o))
        a = b
    if col is None:
        return model(x, **kwargs)   # no graph at all: whatever the model returns for the empty data set
    return _walk(col, None, lambda c, o: c.result(xs))


# ---- evaluate / fit ------------------------------------------------------------------------------------------------------
def evaluate(batch_loss, x, y, batch_size, sample_weight):
    """Mean of ``batch_loss(x_b, y_b, sw_b)`` (a device scalar, or a list of them) over the batches in order, weighted by
    graphs per batch.  The values are read back once, after the last batch."""
    xs, ys, sw = _as_list(x), _as_list(y), _members(sample_weight)
    dev = _device_of(xs)
    ys, sw = resident(ys, dev), None if sw is None else resident(sw, dev)
    G = num_graphs(xs)
    epoch = _Epoch(G, batch_size, False, 0, 0, dev)
    rows, counts = [], []
    for k, ids in enumerate(epoch.ids):
        xb, yb, swb = epoch.take(k, [xs, ys, sw])
        loss = batch_loss(_like(x, xb), _like(y, yb), _like(sample_weight, swb))
        rows.append(torch.stack([v.detach().reshape(()) for v in _as_list(loss)]))
        counts.append(int(ids.shape[0]))
    if not rows:
        raise ValueError("evaluate needs at least one graph")
    table = torch.stack(rows).cpu().numpy()
    means = [weighted_mean(table[:, j], counts) for j in range(table.shape[1])]
    return means if isinstance(loss, (list, tuple)) else means[0]


def fit(model, names, x, y, batch_size=32, epochs=1, shuffle=True, validation_data=None, sample_weight=None,
        callbacks=None, initial_epoch=0, verbose=0, seed=None):
    """The epochs of ``model.fit``: per epoch the batch rule (``data.batching.batch_ids``), one ``train_on_batch`` per
    batch on tensors cut out of the resident data set on the GPU, then ``model.evaluate`` on ``validation_data``.
    ``names``: what ``train_on_batch`` returns (``["loss"]``, or ``["loss", "energy_loss", "force_loss"]``)."""
    xs, ys, sw = _as_list(x), _as_list(y), _members(sample_weight)
    dev = _device_of(xs)
    ys, sw = resident(ys, dev), None if sw is None else resident(sw, dev)
    G = num_graphs(xs)
    if G == 0:
        raise ValueError("fit needs at least one graph")
    if seed is None:
        seed = int(np.random.SeedSequence().generate_state(1)[0])
    history = History()
    history.params = {"batch_size": int(batch_size), "epochs": int(epochs), "steps": -(-G // int(batch_size)),
                      "shuffle": bool(shuffle), "seed": int(seed), "verbose": verbose}
    cbs = list(callbacks or []) + [history]   # the history comes last: it records what the other callbacks logged
    for cb in cbs:
        if hasattr(cb, "set_model"):
            cb.set_model(model)

    def emit(hook, *args):
        for cb in cbs:
            fn = getattr(cb, hook, None)
            if fn is not None:
                fn(*args)

    model.stop_training = False
    emit("on_train_begin", None)
    for ep in range(int(initial_epoch), int(epochs)):
        emit("on_epoch_begin", ep, {})
        batches = _Epoch(G, batch_size, shuffle, seed, ep, dev)
        values, counts = [], []
        for k, ids in enumerate(batches.ids):
            xb, yb, swb = batches.take(k, [xs, ys, sw])
            values.append(_as_list(model.train_on_batch(_like(x, xb), _like(y, yb), _like(sample_weight, swb))))
            counts.append(int(ids.shape[0]))
        logs = {n: weighted_mean([v[j] for v in values], counts) for j, n in enumerate(names)}
        if validation_data is not None:
            val = _as_list(model.evaluate(validation_data[0], validation_data[1], batch_size=batch_size,
                                          sample_weight=validation_data[2] if len(validation_data) > 2 else None))
            logs.update({"val_" + n: v for n, v in zip(names, val)})
        emit("on_epoch_end", ep, logs)
        if verbose:
            print("Epoch %d/%d - %s" % (ep + 1, int(epochs), " - ".join("%s: %.6g" % kv for kv in logs.items())))
        if getattr(model, "stop_training", False):
            break
    emit("on_train_end", None)
    return history
