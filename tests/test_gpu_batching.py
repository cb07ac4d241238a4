"""fit / predict / evaluate over a resident data set with on-GPU batching: ``mp_ragged_take`` bit for bit against NumPy
(it is a copy), ``take_batch``, and the loop (``gcnn_keras_amd/model/loop.py``) against the oracles and against a
hand-written ``train_on_batch`` loop over host-built batches."""
import ctypes

import numpy as np
import pytest
import torch

from gcnn_keras_amd import _ffi, synth
from gcnn_keras_amd.data.batching import batch_ids, take_batch
from gcnn_keras_amd.model.loop import Callback, weighted_mean
from oracle import kgcnn_oracle as ko
from oracle import torch_force_oracle as tfo
from parity import assert_forces_close, assert_rows_close

pytestmark = pytest.mark.gpu

G = 37


def _dev(values, splits):
    from gcnn_keras_amd.ragged import RaggedTensor
    return RaggedTensor.from_numpy(values, splits)


# ------------------------------------------------------------------------------------------------------------- the kernel
_DATASET = {}


def _dataset():
    """37 graphs, row counts from {0, 0, 1, 2, ..., 29}; an empty graph first, one last, two adjacent.  Built once."""
    if _DATASET:
        return _DATASET
    rng = np.random.default_rng(2024)
    pool = np.array([0, 0] + list(range(1, 30)))
    n_len, m_len = rng.choice(pool, size=G), rng.choice(pool, size=G)
    for lens in (n_len, m_len):
        lens[0] = lens[-1] = lens[11] = lens[12] = 0
        lens[1], lens[5], lens[G - 2] = 29, 1, 3
    ns = np.concatenate([[0], np.cumsum(n_len)]).astype(np.int64)
    ms = np.concatenate([[0], np.cumsum(m_len)]).astype(np.int64)
    n, m = int(ns[-1]), int(ms[-1])
    host = [(rng.normal(size=(n,)).astype(np.float32), ns),                       # f32 (N,)
            (rng.normal(size=(n, 3)).astype(np.float32), ns),                     # f32 (N, 3): 12-byte rows
            (rng.integers(-2 ** 40, 2 ** 40, size=(m, 2)).astype(np.int64), ms),  # int64 (M, 2)
            (rng.normal(size=(n, 128)).astype(np.float32), ns),                   # f32 (N, 128)
            (rng.integers(-2 ** 40, 2 ** 40, size=(n,)).astype(np.int64), ns)]    # int64 (N,)
    _DATASET.update(host=host, dev=[_dev(v, s) for v, s in host])
    return _DATASET


def _numpy_take(values, splits, ids):
    lens = (splits[1:] - splits[:-1])[ids]
    out_splits = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows = [values[splits[i]:splits[i + 1]] for i in ids]
    out = np.concatenate(rows, axis=0) if rows else values[:0]
    return out, out_splits


def _check(got, host, ids):
    assert len(got) == len(host)
    for r, (values, splits) in zip(got, host):
        ref, ref_splits = _numpy_take(values, splits, ids)
        assert r.values.dtype == torch.from_numpy(values).dtype and tuple(r.values.shape) == ref.shape
        assert torch.equal(r.values.cpu(), torch.from_numpy(np.ascontiguousarray(ref)))
        assert torch.equal(r.row_splits.cpu(), torch.from_numpy(ref_splits))       # device splits ...
        assert np.array_equal(r._splits_host, ref_splits)                          # ... equal the host-computed ones


def _id_lists():
    rng = np.random.default_rng(7)
    lists = {"identity": np.arange(G), "reversed": np.arange(G)[::-1].copy(), "permutation": rng.permutation(G),
             "repeats": np.array([3, 3, 1, 36, 1, 1, 0, 12, 11, 3]), "one empty": np.array([11]),
             "one non-empty": np.array([1])}
    for B in (63, 64, 65, _ffi.MP_TAKE_SCAN_WIDTH + 1, 5000):      # 1025 = one scan pass + 1; 5000: five passes
        lists["B=%d" % B] = rng.integers(0, G, size=B)
    return lists


@pytest.mark.parametrize("name", list(_id_lists()))
def test_ragged_take_equals_numpy(name):
    d = _dataset()
    ids = _id_lists()[name].astype(np.int64)
    got = take_batch(d["dev"], torch.from_numpy(ids).cuda(), ids)
    _check(got, d["host"], ids)
    one = d["dev"][1].take(ids)                                    # the one-tensor form
    assert torch.equal(one.values, got[1].values) and torch.equal(one.row_splits, got[1].row_splits)


@pytest.mark.parametrize("first", [0, 5, G - 3])
def test_ragged_take_contiguous_range(first):
    d = _dataset()
    for B in (3, 1):
        ids = np.arange(first, first + B)
        got = take_batch(d["dev"], None, ids)                      # take == NULL: the same kernel, no view
        _check(got, d["host"], ids)
        for r, src in zip(got, d["dev"]):
            assert r.values.data_ptr() % 256 == 0 or r.values.numel() == 0
            lo = src.values.data_ptr()
            assert not lo <= r.values.data_ptr() < lo + max(src.values.numel() * src.values.element_size(), 1)
    with pytest.raises(ValueError):
        take_batch(d["dev"], None, np.array([0, 2]))


@pytest.mark.parametrize("offset_bytes", [4, 8, 12])
def test_ragged_take_sources_off_the_16_byte_grid(offset_bytes):
    """Source values that start 4, 8 and 12 bytes into their allocation (pointers passed as they are): the 4-byte path
    next to the 16-byte one."""
    from gcnn_keras_amd.ragged import RaggedTensor
    d = _dataset()
    shifted = []
    for (values, splits), r in zip(d["host"], d["dev"]):
        if values.dtype == np.int64 and offset_bytes % 8:
            shifted.append(r)                                     # an int64 tensor cannot start off an 8-byte boundary
            continue
        lead = offset_bytes // values.dtype.itemsize
        buf = torch.zeros(lead + values.size, dtype=r.values.dtype, device="cuda")
        buf[lead:].copy_(r.values.reshape(-1))
        view = buf[lead:].view(r.values.shape)
        assert view.data_ptr() % 16 == offset_bytes and view.is_contiguous()
        s = RaggedTensor(view, r.row_splits)
        s._splits_host = splits
        shifted.append(s)
    for ids in (np.random.default_rng(9).permutation(G), np.arange(5, 8)):
        ids = ids.astype(np.int64)
        _check(take_batch(shifted, torch.from_numpy(ids).cuda(), ids), d["host"], ids)


def test_ragged_take_destination_off_the_16_byte_grid_and_raw_call():
    """The C call as a host struct, destination values 4 bytes into their allocation: every unit takes the 4-byte path."""
    d = _dataset()
    values, splits = d["host"][1]
    src = d["dev"][1]
    ids = np.array([1, 0, 5, 1, 35, 36, 2], dtype=np.int64)
    ref, ref_splits = _numpy_take(values, splits, ids)
    ids_dev = torch.from_numpy(ids).cuda()
    buf = torch.full((1 + ref.size + 8,), -7.0, device="cuda")
    dst = buf[1:1 + ref.size]
    dst_splits = torch.empty(len(ids) + 1, dtype=torch.int64, device="cuda")
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    desc = _ffi.TakeDesc()
    desc.k, desc.G, desc.B, desc.first, desc.take, desc.flags = 1, G, len(ids), 0, ids_dev.data_ptr(), flags.data_ptr()
    it = desc.item[0]
    it.src_values, it.src_splits, it.row_bytes = src.values.data_ptr(), src.row_splits.data_ptr(), 12
    it.dst_values, it.dst_splits, it.dst_rows = dst.data_ptr(), dst_splits.data_ptr(), ref.shape[0]
    _ffi.call("mp_ragged_take", ctypes.byref(desc), _ffi.stream())
    assert torch.equal(dst.cpu(), torch.from_numpy(ref.reshape(-1)))
    assert torch.equal(dst_splits.cpu(), torch.from_numpy(ref_splits)) and int(flags.item()) == 0
    assert float(buf[0]) == -7.0 and torch.all(buf[1 + ref.size:] == -7.0)       # nothing written around the destination
    # a destination sized too small is never overrun
    buf.fill_(-7.0)
    it.dst_rows = ref.shape[0] - 4
    _ffi.call("mp_ragged_take", ctypes.byref(desc), _ffi.stream())
    keep = (ref.shape[0] - 4) * 3
    assert torch.equal(buf[1:1 + keep].cpu(), torch.from_numpy(ref.reshape(-1)[:keep]))
    assert torch.all(buf[1 + keep:] == -7.0)


def test_ragged_take_out_of_range_ids_clamp_and_flag():
    from gcnn_keras_amd.data import batching
    d = _dataset()
    flags = batching._flag_word(d["dev"][0].values.device)
    for bad, clamped in ((G, G - 1), (-1, 0)):
        ids = np.array([4, bad, 7, 1], dtype=np.int64)
        ids_dev = torch.from_numpy(ids).cuda()
        flags.zero_()
        got = take_batch(d["dev"], ids_dev, ids)                    # the call returns, nothing faults
        torch.cuda.synchronize()
        assert int(flags.item()) & _ffi.MP_FLAG_OOB
        _check(got, d["host"], np.where(ids == bad, clamped, ids))
        with pytest.raises(IndexError):
            take_batch(d["dev"], ids_dev, ids, ragged_validate=True)
        with pytest.raises(IndexError):
            d["dev"][0].take(ids, ragged_validate=True)
    good = np.array([4, 7], dtype=np.int64)
    take_batch(d["dev"], torch.from_numpy(good).cuda(), good, ragged_validate=True)   # validation starts from a clean word
    assert int(flags.item()) == 0


def test_take_batch_dense_members_chunks_and_none():
    d = _dataset()
    rng = np.random.default_rng(5)
    energy = rng.normal(size=(G, 2)).astype(np.float32)
    charge = rng.integers(-3, 4, size=(G,)).astype(np.int64)
    weight = rng.normal(size=(G,)).astype(np.float32)
    members = d["dev"] + [torch.from_numpy(energy).cuda(), None] + d["dev"] + [torch.from_numpy(charge).cuda(),
                                                                               torch.from_numpy(weight).cuda()]
    assert sum(1 for t in members if hasattr(t, "row_splits")) > _ffi.MP_TAKE_MAX   # more than one mp_ragged_take call
    ids = rng.permutation(G)[:9].astype(np.int64)
    for ids_dev, ids_host in ((torch.from_numpy(ids).cuda(), ids), (None, np.arange(30, 37))):
        before = _ffi.launch_count()
        got = take_batch(members, ids_dev, ids_host)
        assert _ffi.launch_count() - before == 2 + 3               # two chunks of ragged members, three dense gathers
        _check(got[:5], d["host"], ids_host)
        _check(got[7:12], d["host"], ids_host)
        assert got[6] is None
        assert torch.equal(got[5].cpu(), torch.from_numpy(energy[ids_host]))
        assert torch.equal(got[12].cpu(), torch.from_numpy(charge[ids_host])) and got[12].dtype == torch.int64
        assert torch.equal(got[13].cpu(), torch.from_numpy(weight[ids_host]))
    empty = take_batch(d["dev"][:2], None, np.zeros(0, np.int64))
    assert empty[1].values.shape == (0, 3) and empty[1].row_splits.cpu().tolist() == [0]


# --------------------------------------------------------------------------------------------------------------- predict
def _schnet(seed=7):
    from gcnn_keras_amd.literature import Schnet
    p = synth.schnet_params(seed=seed, random_bias=True)
    model = Schnet.make_model(depth=3)
    model.set_weights(list(p.values()))
    return p, model


def _mol_inputs(b):
    return [_dev(b["node_number"], b["node_splits"]), _dev(b["node_coordinates"], b["node_splits"]),
            _dev(b["edge_indices"], b["edge_splits"])]


def test_predict_schnet_fused_route():
    b = synth.qm9_like_batch(num_graphs=23, seed=31)
    p, model = _schnet()
    x = _mol_inputs(b)
    whole = model(x)
    assert torch.equal(model.predict(x), whole)                    # no batch_size: today's behaviour, one call
    model.fused.last = None
    out = model.predict(x, batch_size=8)                           # 8, 8, 7
    assert model.fused.last == "direct"                            # every batch is new to the route
    assert tuple(out.shape) == tuple(whole.shape) == (23, 1) and out.dtype == whole.dtype

    def oracle(dtype):
        return ko.schnet_forward(ko.to_dtype(p, dtype), ko.R(b["node_number"], b["node_splits"]),
                                 ko.R(b["node_coordinates"].astype(dtype), b["node_splits"]),
                                 ko.R(b["edge_indices"], b["edge_splits"]), depth=3)

    assert_rows_close(out.cpu().numpy(), oracle(np.float32), oracle(np.float64), what="predict(batch_size=8), SchNet")
    # keyword arguments reach every model call: the layer path
    layers = model.predict(x, batch_size=8, fused=False)
    assert_rows_close(layers.cpu().numpy(), oracle(np.float32), oracle(np.float64), what="predict, SchNet layer path")
    assert tuple(model.predict(x, batch_size=64).shape) == (23, 1)  # one short batch


def _two_size_md17(sizes, seed):
    """MD17-shaped molecules (aspirin composition, cutoff 5 A, every neighbour) of the given atom counts."""
    rng = np.random.default_rng(seed)
    zs, xs, es = [], [], []
    for n in sizes:
        xyz = rng.normal(0.0, 1.7, size=(n, 3)).astype(np.float32)
        zs.append(synth.ASPIRIN_Z[:n].copy()); xs.append(xyz)
        es.append(synth.radius_graph(xyz, max_distance=5.0, max_neighbours=10000))
    return {"node_number": np.concatenate(zs), "node_coordinates": np.concatenate(xs, axis=0),
            "edge_indices": np.concatenate(es, axis=0).reshape(-1, 2).astype(np.int64),
            "node_splits": synth._splits(sizes), "edge_splits": synth._splits([len(e) for e in es])}


def test_predict_painn_energy_force_padded():
    from gcnn_keras_amd.literature import PAiNN
    from gcnn_keras_amd.model.force import EnergyForceModel
    from helpers import painn_weight_list
    sizes = [13, 13, 13, 13, 21, 13, 21, 13, 13, 21, 13]           # the first batch is narrower than the second
    b = _two_size_md17(sizes, seed=5)
    p = synth.painn_params(seed=8, random_bias=True)
    energy = PAiNN.make_model(equiv_initialize_kwargs={"dim": 3, "method": "eps"})
    energy.set_weights(painn_weight_list(p))
    model = EnergyForceModel(model_energy=energy, coordinate_input=1, energy_output=0, output_as_dict=True,
                             output_to_tensor=True, output_squeeze_states=True)
    x = _mol_inputs(b)
    out = model.predict(x, batch_size=4)
    assert set(out) == {"energy", "force"}
    eng, force = out["energy"].cpu().numpy(), out["force"].cpu().numpy()
    assert eng.shape == (11, 1) and force.shape == (11, 21, 3)
    whole = model(x)
    assert tuple(whole["force"].shape) == force.shape and tuple(whole["energy"].shape) == eng.shape
    ns = b["node_splits"]
    flat = np.concatenate([force[g, :sizes[g]] for g in range(11)], axis=0)
    for g in range(11):
        assert np.count_nonzero(force[g, sizes[g]:]) == 0          # zeros in the padding

    def energy_fn(dtype):
        return ko.painn_forward(ko.to_dtype(p, dtype), ko.R(b["node_number"], ns),
                                ko.R(b["node_coordinates"].astype(dtype), ns), ko.R(b["edge_indices"], b["edge_splits"]),
                                depth=3, equiv_method="eps")

    assert_rows_close(eng, energy_fn(np.float32), energy_fn(np.float64), what="predict PaiNN energy")
    f32, f64 = (tfo.painn_energy_force(p, b, dt, equiv_method="eps")[1] for dt in (torch.float32, torch.float64))
    assert_forces_close(flat, f32, f64, ns, what="predict PaiNN forces, batches of 4")
    # ragged force output: values concatenated, the coordinates' splits
    model.output_to_tensor = False
    rag = model.predict(x, batch_size=4)["force"]
    assert any(rag.row_splits is t.row_splits for t in x[:2]) and tuple(rag.values.shape) == (int(ns[-1]), 3)
    assert_forces_close(rag.values.cpu().numpy(), f32, f64, ns, what="predict PaiNN forces, ragged")


def test_predict_gin_layer_path():
    """``GIN.make_model`` as tests/test_gpu_models.py::test_gin_builder_forward holds it, served in batches."""
    from gcnn_keras_amd.literature import GIN
    b = synth.qm9_like_batch(num_graphs=23, seed=29)
    rng = np.random.default_rng(30)
    n = int(b["node_splits"][-1])
    fn, units, depth, classes = 9, 16, 2, 3
    feat = rng.normal(size=(n, fn)).astype(np.float32)
    model = GIN.make_model(
        inputs=[{"shape": (None, fn), "name": "node_attributes", "dtype": "float32", "ragged": True},
                {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True}],
        gin_mlp={"units": [units, units]}, gin_args={"epsilon_learnable": True}, depth=depth,
        last_mlp={"units": [12, 12, 8]}, output_mlp={"units": classes})
    p, arrays = {}, []
    arrays += [w.cpu().numpy() for _, w in model.layers[0].weights]

    def dense_pair(key, fin, fout):
        p[key + "/kernel"] = synth.glorot_uniform(rng, fin, fout)
        p[key + "/bias"] = (rng.normal(size=fout) * 0.1).astype(np.float32)
        arrays.extend([p[key + "/kernel"], p[key + "/bias"]])

    dense_pair("dense0", fn, units)
    for i in range(depth):
        p["gin%d/eps" % i] = np.float32(0.1 * (i + 1))
        arrays.append(p["gin%d/eps" % i])
        dense_pair("mlp%d/0" % i, units, units)
        dense_pair("mlp%d/1" % i, units, units)
    for j in range(depth + 1):
        dense_pair("last%d/0" % j, units, 12)
        dense_pair("last%d/1" % j, 12, 12)
        dense_pair("last%d/2" % j, 12, 8)
    dense_pair("output", 8, classes)
    model.set_weights(arrays)
    x = [_dev(feat, b["node_splits"]), _dev(b["edge_indices"], b["edge_splits"])]
    out = model.predict(x, batch_size=8)
    assert tuple(out.shape) == tuple(model(x).shape) == (23, classes)
    ref = ko.gin_forward(p, ko.R(feat, b["node_splits"]), ko.R(b["edge_indices"], b["edge_splits"]), depth=depth)
    assert np.max(np.abs(out.cpu().numpy() - ref)) <= 2e-5


# ------------------------------------------------------------------------------------------------------ fit and evaluate
def _host_batch(b, ids, int_numbers=False):
    """The graphs ``ids`` of a synth batch, concatenated on the host: NumPy slices -> ``RaggedTensor.from_numpy``."""
    ns, es = b["node_splits"], b["edge_splits"]
    z = b["node_number"].astype(np.int64) if int_numbers else b["node_number"]
    n_len, e_len = (ns[1:] - ns[:-1])[ids], (es[1:] - es[:-1])[ids]
    nsp, esp = synth._splits(n_len), synth._splits(e_len)
    cat = lambda a, s: np.concatenate([a[s[i]:s[i + 1]] for i in ids], axis=0)
    return [_dev(cat(z, ns), nsp), _dev(cat(b["node_coordinates"], ns), nsp), _dev(cat(b["edge_indices"], es), esp)], nsp


def _weights_equal(a, c):
    return all(torch.equal(s, t) for s, t in zip(a.trainable_weights, c.trainable_weights))


@pytest.mark.parametrize("shuffle,seed", [(False, None), (True, 3)])
def test_fit_schnet_equals_the_hand_written_loop(shuffle, seed):
    b = synth.qm9_like_batch(num_graphs=19, seed=41)
    target = np.random.default_rng(4).normal(size=(19, 1)).astype(np.float32)
    (_, model), (_, twin) = _schnet(), _schnet()
    model.compile(optimizer="sgd", loss="mean_absolute_error")
    twin.compile(optimizer="sgd", loss="mean_absolute_error")
    hist = model.fit(_mol_inputs(b), torch.from_numpy(target).cuda(), batch_size=8, epochs=2, shuffle=shuffle, seed=seed)
    assert hist.epoch == [0, 1] and hist.params["shuffle"] is shuffle
    used = hist.params["seed"]
    assert isinstance(used, int) and (seed is None or used == seed)
    want = []
    for epoch in range(2):
        ids_of = batch_ids(19, 8, shuffle=shuffle, seed=used, epoch=epoch)
        assert [len(i) for i in ids_of] == [8, 8, 3]
        losses = [twin.train_on_batch(_host_batch(b, ids)[0], target[ids]) for ids in ids_of]
        want.append(weighted_mean(losses, [len(i) for i in ids_of]))
        assert want[-1] == pytest.approx(sum(v * len(i) for v, i in zip(losses, ids_of)) / 19.0, rel=1e-12)
    assert _weights_equal(model, twin)                             # deterministic kernels on the same bits
    assert hist.history["loss"] == want and set(hist.history) == {"loss"}
    assert not any(t.requires_grad for t in model.trainable_weights)


LOSS_WEIGHTS = [1.0 / 200.0, 199.0 / 200.0]   # the fork's force_schnet.py


def _fork_case(num_graphs, seed):
    from gcnn_keras_amd.literature import Schnet
    from gcnn_keras_amd.model.force import EnergyForceModel
    from test_gpu_forces import FORK_SCHNET
    b = synth.md17_like_batch(num_graphs=num_graphs, seed=seed)
    p = synth.schnet_params(seed=7, depth=6, emb_out=128, bins=25, last_units=(128, 64, 1), out_units=(), random_bias=True)

    def build():
        model = Schnet.make_model(**FORK_SCHNET)
        model.set_weights(list(p.values()))
        efm = EnergyForceModel(model_energy=model, coordinate_input=1, energy_output=0, output_as_dict=False,
                               output_to_tensor=False, output_squeeze_states=True, is_physical_force=False)
        efm.compile(optimizer=torch.optim.SGD(efm.trainable_weights, lr=1e-3),
                    loss=["mean_squared_error", "mean_squared_error"], loss_weights=LOSS_WEIGHTS, clipnorm=1.0)
        return efm

    rng = np.random.default_rng(seed + 1)
    e_t = rng.normal(size=(num_graphs, 1)).astype(np.float32)
    f_t = rng.normal(size=(int(b["node_splits"][-1]), 3)).astype(np.float32)
    x = [_dev(b["node_number"].astype(np.int64), b["node_splits"]), _dev(b["node_coordinates"], b["node_splits"]),
         _dev(b["edge_indices"], b["edge_splits"])]
    return b, build, x, e_t, f_t


@pytest.mark.parametrize("shuffle,seed", [(False, None), (True, 3)])
def test_fit_schnet_with_forces_equals_the_hand_written_loop(shuffle, seed):
    b, build, x, e_t, f_t = _fork_case(19, 21)
    efm, twin = build(), build()
    ns = b["node_splits"]
    y = [torch.from_numpy(e_t).cuda(), _dev(f_t, ns)]
    hist = efm.fit(x, y, batch_size=8, epochs=2, shuffle=shuffle, seed=seed)
    used = hist.params["seed"]
    want = {"loss": [], "energy_loss": [], "force_loss": []}
    for epoch in range(2):
        ids_of = batch_ids(19, 8, shuffle=shuffle, seed=used, epoch=epoch)
        rows = []
        for ids in ids_of:
            xb, nsp = _host_batch(b, ids, int_numbers=True)
            fb = np.concatenate([f_t[ns[i]:ns[i + 1]] for i in ids], axis=0)
            rows.append(twin.train_on_batch(xb, [e_t[ids], _dev(fb, nsp)]))
        for j, name in enumerate(want):
            want[name].append(weighted_mean([r[j] for r in rows], [len(i) for i in ids_of]))
    assert _weights_equal(efm, twin)
    assert hist.history == want
    assert not any(t.requires_grad for t in efm.trainable_weights)


def test_evaluate_and_validation_data():
    b = synth.qm9_like_batch(num_graphs=19, seed=41)
    target = np.random.default_rng(4).normal(size=(19, 1)).astype(np.float32)
    weight = np.random.default_rng(5).uniform(0.5, 2.0, size=(19,)).astype(np.float32)
    _, model = _schnet()
    # lr 1e-5: the squared error of random targets is ~40 at the start and Keras' SGD default (0.01) diverges on it
    model.compile(optimizer=torch.optim.SGD(model.trainable_weights, lr=1e-5), loss="mean_squared_error")
    x, y = _mol_inputs(b), torch.from_numpy(target).cuda()
    before = [t.clone() for t in model.trainable_weights]
    got = model.evaluate(x, y, batch_size=8)
    got_w = model.evaluate(x, y, batch_size=8, sample_weight=weight)
    assert all(torch.equal(s, t) and not t.requires_grad for s, t in zip(before, model.trainable_weights))
    pred = model.predict(x, batch_size=8)
    cuts = [(0, 8), (8, 16), (16, 19)]
    per = [float(model._loss_fn(pred[a:c], y[a:c], None)) for a, c in cuts]
    per_w = [float(model._loss_fn(pred[a:c], y[a:c], weight[a:c])) for a, c in cuts]
    assert got == weighted_mean(per, [8, 8, 3]) and got_w == weighted_mean(per_w, [8, 8, 3])
    assert isinstance(got, float) and got != got_w

    seen = []

    class AfterEpoch(Callback):
        def on_epoch_end(self, epoch, logs=None):
            seen.append((logs["val_loss"], self.model.evaluate(x, y, batch_size=8)))

    hist = model.fit(x, y, batch_size=8, epochs=2, shuffle=True, seed=1, validation_data=(x, y), callbacks=[AfterEpoch()])
    assert hist.history["val_loss"] == [v for v, _ in seen] == [e for _, e in seen]   # evaluate after that epoch
    assert np.all(np.isfinite(hist.history["val_loss"])) and np.all(np.isfinite(hist.history["loss"]))
    assert hist.history["val_loss"][0] != got and set(hist.history) == {"loss", "val_loss"}


def test_evaluate_energy_force_model():
    b, build, x, e_t, f_t = _fork_case(11, 33)
    efm = build()
    efm.fused = False                                              # predict on the tape: the pass evaluate runs
    ns = b["node_splits"]
    y = [torch.from_numpy(e_t).cuda(), _dev(f_t, ns)]
    before = [t.clone() for t in efm.trainable_weights]
    got = efm.evaluate(x, y, batch_size=4)
    assert all(torch.equal(s, t) and not t.requires_grad for s, t in zip(before, efm.trainable_weights))
    eng, force = efm.predict(x, batch_size=4)
    rows = []
    for a, c in [(0, 4), (4, 8), (8, 11)]:
        le = float(efm._loss_fns[0](eng[a:c], y[0][a:c], None))
        lf = float(efm._loss_fns[1](force.values[ns[a]:ns[c]], y[1].values[ns[a]:ns[c]], None))
        total = float(torch.tensor(le, dtype=torch.float32) * LOSS_WEIGHTS[0]
                      + torch.tensor(lf, dtype=torch.float32) * LOSS_WEIGHTS[1])
        rows.append([total, le, lf])
    want = [weighted_mean([r[j] for r in rows], [4, 4, 3]) for j in range(3)]
    assert got[1:] == want[1:] and got[0] == pytest.approx(want[0], rel=1e-6)
    hist = efm.fit(x, y, batch_size=4, epochs=1, shuffle=False, validation_data=(x, y))
    assert set(hist.history) == {"loss", "energy_loss", "force_loss", "val_loss", "val_energy_loss", "val_force_loss"}
    after = efm.evaluate(x, y, batch_size=4)
    assert [hist.history["val_" + n][0] for n in ("loss", "energy_loss", "force_loss")] == after


def test_scheduler_and_stop_training_in_fit():
    from gcnn_keras_amd.training.scheduler import LinearLearningRateScheduler
    b = synth.qm9_like_batch(num_graphs=9, seed=43)
    target = np.zeros((9, 1), np.float32)
    _, model = _schnet()
    model.compile(optimizer="sgd", loss="mean_absolute_error")
    sched = LinearLearningRateScheduler(learning_rate_start=1e-3, learning_rate_stop=1e-4, epo_min=1, epo=3)
    rates = []

    class Watch(Callback):
        def on_epoch_begin(self, epoch, logs=None):
            rates.append([g["lr"] for g in self.model.optimizer.param_groups])

        def on_epoch_end(self, epoch, logs=None):
            if epoch == 3:
                self.model.stop_training = True

    hist = model.fit(_mol_inputs(b), target, batch_size=8, epochs=6, callbacks=[sched, Watch()], seed=0)
    want = [1e-3, 1e-3, 1e-3 - (1e-3 - 1e-4) / 2.0, 1e-4]
    assert hist.epoch == [0, 1, 2, 3]                              # stop_training ends fit after that epoch
    assert hist.history["lr"] == pytest.approx(want, rel=1e-12)
    assert [r[0] for r in rates] == pytest.approx(want, rel=1e-12) and all(len(set(r)) == 1 for r in rates)
    assert len(hist.history["loss"]) == 4


def test_fit_on_a_builder_that_refuses_trainable_weights():
    from gcnn_keras_amd.literature import PAiNN
    b = synth.md17_like_batch(num_graphs=3, seed=5)
    model = PAiNN.make_model(equiv_initialize_kwargs={"dim": 3, "method": "eps"})
    model.compile(optimizer="sgd", loss="mean_absolute_error")
    with pytest.raises(NotImplementedError):
        model.fit(_mol_inputs(b), np.zeros((3, 1), np.float32), batch_size=2, epochs=1)
    assert not any(t.requires_grad for t in model.trainable_weights)
    with pytest.raises(RuntimeError):
        PAiNN.make_model(equiv_initialize_kwargs={"dim": 3, "method": "eps"}).fit(_mol_inputs(b), np.zeros((3, 1)))
