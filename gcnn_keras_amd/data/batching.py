"""Batches of a resident data set, assembled on the GPU.

``MemoryGraphList.tensor(...)`` returns the whole data set as device ``RaggedTensor``s; that is the resident data set.
``take_batch`` cuts the graphs ``ids`` out of it: every ragged member through ONE ``mp_ragged_take`` call (the analogue of
``tf.gather(ragged, ids)``, csrc/mp_take.hip), dense per-graph members (energies, total charges, sample weights) through
the row gather.  Output sizes come from the host copy of the row splits, so no batch costs a device-to-host copy or a
stream synchronisation, and a shuffled epoch (``model.fit(..., shuffle=True)``, kgcnn/training/train_qm.py:159-166) is not
fed by the host packer.

``batch_ids`` is the batch rule of an epoch and part of the interface:

* ``ceil(G / batch_size)`` batches, the short last one kept (Keras),
* ``shuffle=False``: ``arange(G)`` cut in order,
* ``shuffle=True``: ``np.random.default_rng([seed, epoch]).permutation(G)`` cut in order.
"""
import ctypes

import numpy as np
import torch

from .. import _ffi
from ..ragged import RaggedTensor

_flag_words = {}


def _flag_word(device):
    """One int32 flag word per device (``MP_FLAG_OOB`` is ORed into it); zeroed only when a caller asks to validate."""
    word = _flag_words.get(device)
    if word is None:
        word = _flag_words[device] = torch.zeros(1, dtype=torch.int32, device=device)
    return word


def batch_ids(G, batch_size, shuffle=False, seed=0, epoch=0):
    """The graph ids of every batch of one epoch: a list of int64 arrays."""
    G, batch_size = int(G), int(batch_size)
    if batch_size < 1:
        raise ValueError("batch_size must be positive, got %r" % (batch_size,))
    if shuffle:
        order = np.random.default_rng([int(seed), int(epoch)]).permutation(G).astype(np.int64)
    else:
        order = np.arange(G, dtype=np.int64)
    return [order[a:a + batch_size] for a in range(0, G, batch_size)]


def num_graphs(tensors):
    """Number of graphs of a resident data set (its first member's leading axis)."""
    for t in tensors if isinstance(tensors, (list, tuple)) else [tensors]:
        if isinstance(t, RaggedTensor):
            return t.nrows()
        if torch.is_tensor(t):
            return int(t.shape[0])
    raise ValueError("no tensor to take the number of graphs from")


def _row_bytes(values):
    n = values.element_size()
    for d in values.shape[1:]:
        n *= int(d)
    return n


def _take_ragged(members, ids_device, ids_host, first, validate):
    """``mp_ragged_take`` over ``members`` (at most ``MP_TAKE_MAX``); ids_host is already clamped into [0, G)."""
    B = int(ids_host.shape[0])
    G = members[0].nrows()
    dev = members[0].values.device
    desc = _ffi.TakeDesc()
    desc.k, desc.G, desc.B, desc.first = len(members), G, B, int(first)
    desc.take = None if ids_device is None else ids_device.data_ptr()
    flags = _flag_word(dev)
    if validate:
        flags.zero_()
    desc.flags = flags.data_ptr()
    out, keep = [], []
    for i, r in enumerate(members):
        _ffi.require_device(r.values, r.row_splits)
        if r.nrows() != G:
            raise ValueError("ragged members of one data set must share their graph axis: %d vs %d graphs" % (r.nrows(), G))
        rb = _row_bytes(r.values)
        if rb % 4 != 0 or rb == 0:
            raise TypeError("rows of %d bytes (%s): the take kernel moves 4-byte words" % (rb, r.values.dtype))
        src = r.values if r.values.is_contiguous() else r.values.contiguous()
        splits = r.row_splits_host()
        lens = (splits[1:] - splits[:-1])[ids_host]
        dst_splits_host = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(lens, out=dst_splits_host[1:])
        rows = int(dst_splits_host[-1])
        values = torch.empty((rows,) + tuple(src.shape[1:]), dtype=src.dtype, device=dev)
        # B == 0: the engine returns without a launch, the one split is written here
        dst_splits = (torch.empty if B else torch.zeros)(B + 1, dtype=torch.int64, device=dev)
        it = desc.item[i]
        it.src_values, it.src_splits, it.row_bytes = src.data_ptr(), r.row_splits.data_ptr(), rb
        it.dst_values, it.dst_splits, it.dst_rows = values.data_ptr(), dst_splits.data_ptr(), rows
        keep.append(src)   # a contiguous copy must outlive the loop: its block would go to the next allocation
        res = RaggedTensor(values, dst_splits)
        res._splits_host = dst_splits_host
        out.append(res)
    _ffi.call("mp_ragged_take", ctypes.byref(desc), _ffi.stream())
    if validate and int(flags.item()) & _ffi.MP_FLAG_OOB:
        raise IndexError("graph id out of range for a data set of %d graphs" % G)
    return out


def _take_dense(t, ids_i32, B):
    """Rows ``ids`` of a dense per-graph tensor ``(G, ...)`` through the engine's row gather (a bit-exact copy, so any
    element type of 4 or 8 bytes travels as float32 words)."""
    _ffi.require_device(t)
    if t.element_size() % 4 != 0:
        raise TypeError("dense members must have 4- or 8-byte elements, got %s" % t.dtype)
    G = int(t.shape[0])
    src = t.contiguous().reshape(G, -1).view(torch.float32)
    out = torch.empty((B,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    if B and src.shape[1]:
        _ffi.call("mp_gather_rows_f32", _ffi.ptr(src), G, int(src.shape[1]), _ffi.ptr(ids_i32), B, 1,
                  _ffi.int32_array([0]), _ffi.ptr(out), _ffi.stream())
    return out


def take_batch(tensors, ids_device, ids_host, ids_device_i32=None, ragged_validate=False):
    """The graphs ``ids`` of the resident data set ``tensors`` (a list of ``RaggedTensor`` and dense ``(G, ...)`` device
    tensors; ``None`` members stay ``None``) as a list of fresh tensors.

    ``ids_host``: the ids as a host array (sizes are computed from it).  ``ids_device``: the same ids as a device int64
    tensor, or ``None`` for the contiguous range ``ids_host[0] .. ids_host[0] + B - 1``.  ``ids_device_i32``: the ids as
    device int32 for the dense members (made from ``ids_device`` when not given).  An id outside ``[0, G)`` is clamped
    (ragged members) or reads as zeros (dense members) and never faults; ``ragged_validate=True`` reads the flag word back
    and raises ``IndexError`` (the one synchronising option)."""
    ids_host = np.asarray(ids_host, dtype=np.int64).reshape(-1)
    B = int(ids_host.shape[0])
    first = int(ids_host[0]) if B else 0
    if ids_device is None:
        if B and not np.array_equal(ids_host, np.arange(first, first + B, dtype=np.int64)):
            raise ValueError("ids that are no contiguous range need their device copy (ids_device)")
    else:
        _ffi.require_device(ids_device)
        if ids_device.dtype != torch.int64 or tuple(ids_device.shape) != (B,):
            raise ValueError("ids_device must be int64 with one entry per id")
    ragged = [i for i, t in enumerate(tensors) if isinstance(t, RaggedTensor)]
    out = list(tensors)
    if ragged:
        G = tensors[ragged[0]].nrows()
        if G == 0 and B:
            raise IndexError("graph ids asked of an empty data set")
        clamped = np.clip(ids_host, 0, max(G - 1, 0))
        for lo in range(0, len(ragged), _ffi.MP_TAKE_MAX):
            chunk = ragged[lo:lo + _ffi.MP_TAKE_MAX]
            for i, r in zip(chunk, _take_ragged([tensors[i] for i in chunk], ids_device, clamped, first,
                                                ragged_validate)):
                out[i] = r
    ids32 = ids_device_i32
    for i, t in enumerate(tensors):
        if t is None or isinstance(t, RaggedTensor):
            continue
        if not torch.is_tensor(t):
            raise TypeError("members of a resident data set are RaggedTensor or device tensors, got %s" % type(t).__name__)
        if ids32 is None:
            ids32 = (torch.arange(first, first + B, dtype=torch.int32, device=t.device) if ids_device is None
                     else ids_device.to(torch.int32))
        out[i] = _take_dense(t, ids32, B)
    return out
