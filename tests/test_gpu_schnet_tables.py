"""SchNet stage 0 on the node-input tables (csrc/mp_schnet_table.hip): the rows the input chain writes for every node
number, gathered per node instead of recomputed.  Everything here is compared bit for bit: a table row is written by the
chain itself."""
import numpy as np
import pytest
import torch

from gcnn_keras_amd import synth
from oracle import kgcnn_oracle as ko
from parity import assert_rows_close

pytestmark = pytest.mark.gpu

VOCAB = 95
BUILDS = {"node": 3, "node_bf": 3 | 64}      # flags of the FP32 and of the bf16-piece node build (bit 0: fast softplus)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _device_params(emb_out=64, bias=True, seed=7):
    p = synth.schnet_params(seed=seed, emb_in=VOCAB, emb_out=emb_out, random_bias=bias)
    if not bias:
        p = {k: v for k, v in p.items() if k != "dense0/bias"}
    return {k: _cuda(v) for k, v in p.items()}


def _images(p):
    from gcnn_keras_amd.fused import pack_weights
    return pack_weights(p, 3, 20)


def _chain(p, images, build, numbers):
    """n, x of ``mp_schnet_node_in_f32`` for ``numbers`` (float32 or int64 device tensor)."""
    from gcnn_keras_amd import _ffi
    N = int(numbers.shape[0])
    n = torch.full((max(N, 1), 128), 7.0, device="cuda")
    x = torch.full((max(N, 1), 128), 7.0, device="cuda")
    w = images[build]
    flags = BUILDS[build] | (256 if numbers.dtype == torch.int64 else 0)
    _ffi.call("mp_schnet_node_in_f32", _ffi.ptr(numbers), N, _ffi.ptr(p["embedding"]), VOCAB,
              int(p["embedding"].shape[1]), _ffi.ptr(w["dense0/kernel"]), _ffi.ptr(p.get("dense0/bias")),
              _ffi.ptr(w["interaction0/dense1/kernel"]), _ffi.ptr(n), _ffi.ptr(x), flags, _ffi.stream())
    return n, x


def _gather(images, build, numbers):
    from gcnn_keras_amd import _ffi
    N = int(numbers.shape[0])
    n = torch.full((max(N, 1), 128), 7.0, device="cuda")
    x = torch.full((max(N, 1), 128), 7.0, device="cuda")
    t = images["table"][build]
    flags = BUILDS[build] | (256 if numbers.dtype == torch.int64 else 0)
    _ffi.call("mp_schnet_node_in_table_f32", _ffi.ptr(numbers), N, VOCAB, _ffi.ptr(t[0]), _ffi.ptr(t[1]), _ffi.ptr(n),
              _ffi.ptr(x), flags, _ffi.stream())
    return n, x


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("i64", [False, True])
@pytest.mark.parametrize("emb_out", [64, 128])
def test_table_rows_are_the_chain_rows(emb_out, i64, bias):
    """Numbers at both ends of the vocabulary, outside it (-1, vocab, 1000) and, as float32, between two integers; N at
    the tile edges of the chain (0, 1, 15, 16, 17, 33); with a random ``dense0/bias`` and without one; both node builds."""
    p = _device_params(emb_out, bias)
    images = _images(p)
    special = [0, VOCAB - 1, -1, VOCAB, 1000, 5 if i64 else 5.7, 1, 6, 8, 94, 93, -7, 2 ** 31 + 3 if i64 else 94.5]
    rng = np.random.default_rng(3)
    pool = np.asarray(special + list(rng.integers(0, VOCAB, size=33)), dtype=np.int64 if i64 else np.float32)
    for build in BUILDS:
        t = images["table"][build]
        assert tuple(t.shape) == (2, VOCAB + 1, 128)
        cases = [pool[:n] for n in (0, 15, 16, 17, 33)] + [pool[k:k + 1] for k in range(len(special))]
        for numbers in cases:
            z = _cuda(numbers)
            n_ref, x_ref = _chain(p, images, build, z)
            n_got, x_got = _gather(images, build, z)
            torch.cuda.synchronize()
            assert torch.equal(n_got, n_ref) and torch.equal(x_got, x_ref), (build, numbers[:8])


def _edge_prepare(z_like, b):
    from gcnn_keras_amd import _ffi
    M, G, N = int(b["idx"].shape[0]), int(b["ns"].shape[0]) - 1, int(z_like.shape[0])
    recv = torch.full((max(M, 1),), -3, dtype=torch.int32, device="cuda")
    send = torch.full((max(M, 1),), -3, dtype=torch.int32, device="cuda")
    dist = torch.full((max(M, 1),), -3.0, device="cuda")
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    _ffi.call("mp_edge_prepare_i64_f32", _ffi.ptr(b["idx"]), M, _ffi.ptr(b["ns"]), _ffi.ptr(b["es"]), G, N,
              _ffi.ptr(b["xyz"]), _ffi.ptr(recv), _ffi.ptr(send), _ffi.ptr(dist), _ffi.ptr(flags), _ffi.stream())
    return recv, send, dist, flags


def _stage0_table(images, build, b):
    from gcnn_keras_amd import _ffi
    M, G, N = int(b["idx"].shape[0]), int(b["ns"].shape[0]) - 1, int(b["z"].shape[0])
    recv = torch.full((max(M, 1),), -3, dtype=torch.int32, device="cuda")
    send = torch.full((max(M, 1),), -3, dtype=torch.int32, device="cuda")
    dist = torch.full((max(M, 1),), -3.0, device="cuda")
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    n = torch.full((max(N, 1), 128), 7.0, device="cuda")
    x = torch.full((max(N, 1), 128), 7.0, device="cuda")
    t = images["table"][build]
    fl = BUILDS[build] | (256 if b["z"].dtype == torch.int64 else 0)
    _ffi.call("mp_schnet_stage0_table_f32", _ffi.ptr(b["z"]), N, VOCAB, _ffi.ptr(t[0]), _ffi.ptr(t[1]), _ffi.ptr(n),
              _ffi.ptr(x), _ffi.ptr(b["idx"]), M, _ffi.ptr(b["ns"]), _ffi.ptr(b["es"]), G, _ffi.ptr(b["xyz"]),
              _ffi.ptr(recv), _ffi.ptr(send), _ffi.ptr(dist), _ffi.ptr(flags), fl, _ffi.stream())
    return recv, send, dist, flags, n, x


def _resident(b):
    return {"z": _cuda(b["node_number"]), "xyz": _cuda(b["node_coordinates"]), "idx": _cuda(b["edge_indices"]),
            "ns": _cuda(b["node_splits"]), "es": _cuda(b["edge_splits"])}


def _without_edges(b):
    b = dict(b)
    b["edge_indices"] = np.zeros((0, 2), np.int64)
    b["edge_splits"] = np.zeros_like(b["edge_splits"])
    return b


def _break_order(b):
    b = dict(b)
    idx = b["edge_indices"].copy()
    lo, hi = int(b["edge_splits"][-2]), int(b["edge_splits"][-1])     # last graph: last receiver first
    idx[lo:hi] = idx[lo:hi][::-1]
    b["edge_indices"] = idx
    return b


def _out_of_range(b):
    b = dict(b)
    idx = b["edge_indices"].copy()
    idx[-1, 1] = 1000
    b["edge_indices"] = idx
    return b


STAGE0_CASES = {
    "six_graphs": lambda: synth.qm9_like_batch(num_graphs=6, seed=11),
    "one_graph": lambda: synth.qm9_like_batch(num_graphs=1, seed=11),
    "no_edges": lambda: _without_edges(synth.qm9_like_batch(num_graphs=6, seed=11)),
    "six_graphs_unsorted": lambda: _break_order(synth.qm9_like_batch(num_graphs=6, seed=11)),
    "six_graphs_out_of_range": lambda: _out_of_range(synth.qm9_like_batch(num_graphs=6, seed=11)),
    # more edges than the 128 x 256 threads of the edge role: the build with four edges of a thread in flight
    "many_edges": lambda: synth.qm9_like_batch(num_graphs=200, seed=12),
    "many_edges_unsorted": lambda: _break_order(synth.qm9_like_batch(num_graphs=200, seed=12)),
    "many_edges_out_of_range": lambda: _out_of_range(synth.qm9_like_batch(num_graphs=200, seed=12)),
}


@pytest.mark.parametrize("case", list(STAGE0_CASES))
def test_stage0_table_equals_edge_prepare_and_chain(case):
    from gcnn_keras_amd import _ffi
    b = STAGE0_CASES[case]()
    if case.startswith("many_edges"):
        assert 128 * 256 < len(b["edge_indices"]) < 4 * 128 * 256 and len(b["node_number"]) <= 1024 * 16
    p = _device_params()
    images = _images(p)
    r = _resident(b)
    want = (_ffi.MP_FLAG_UNSORTED_COL0 if case.endswith("unsorted") else 0) | \
           (_ffi.MP_FLAG_OOB if case.endswith("out_of_range") else 0)
    for build in BUILDS:
        recv, send, dist, flags, n, x = _stage0_table(images, build, r)
        recv0, send0, dist0, flags0 = _edge_prepare(r["z"], r)
        n0, x0 = _chain(p, images, build, r["z"])
        torch.cuda.synchronize()
        assert torch.equal(recv, recv0) and torch.equal(send, send0) and torch.equal(dist, dist0)
        assert torch.equal(flags, flags0) and int(flags.item()) == want
        assert torch.equal(n, n0) and torch.equal(x, x0)


def _model(p):
    from gcnn_keras_amd.literature import Schnet
    model = Schnet.make_model(depth=3)
    model.set_weights(list(p.values()))
    return model


def _oracle(p, b):
    return ko.schnet_forward(p, ko.R(b["node_number"], b["node_splits"]), ko.R(b["node_coordinates"], b["node_splits"]),
                             ko.R(b["edge_indices"], b["edge_splits"]), depth=3)


def _unsorted(b, seed=1):
    rng = np.random.default_rng(seed)
    b = dict(b)
    idx = b["edge_indices"].copy()
    for g in range(len(b["edge_splits"]) - 1):
        lo, hi = b["edge_splits"][g], b["edge_splits"][g + 1]
        idx[lo:hi] = idx[lo:hi][rng.permutation(hi - lo)]
    b["edge_indices"] = idx
    return b


@pytest.mark.parametrize("shuffle", [False, True])
def test_switch_off_keeps_the_chain_and_the_bits(shuffle, monkeypatch):
    """``MPENGINE_NODE_TABLE=0``: the chain runs; same output bits on the 6-graph batch.  ``shuffle``: receivers out of
    order - the slot's sort branch, whose node rows come from the stand-alone gather launch."""
    from helpers import mol_inputs
    b = synth.qm9_like_batch(num_graphs=6, seed=11)
    if shuffle:
        b = _unsorted(b)
    p = synth.schnet_params(seed=7, random_bias=True)
    outs = {}
    for env in ("1", "0"):
        monkeypatch.setenv("MPENGINE_NODE_TABLE", env)
        model = _model(p)
        x = mol_inputs(b)
        first, second = model(x), model(x)
        torch.cuda.synchronize()
        slot = model.fused.slot_of(x)
        assert (slot.table is not None) == (env == "1") and slot.sorted == (not shuffle)
        assert torch.equal(first, second)
        model.fused.check_flags()
        outs[env] = first
    assert torch.equal(outs["1"], outs["0"])
    assert_rows_close(outs["1"].cpu().numpy(), _oracle(p, b), what="stage 0 on the tables")


def test_weight_updates_reach_the_tables():
    from gcnn_keras_amd import _ffi
    from helpers import mol_inputs
    b = synth.qm9_like_batch(num_graphs=6, seed=11)
    p = synth.schnet_params(seed=7, random_bias=True)
    model = _model(p)
    x = mol_inputs(b)
    old = model(x)
    model(x)
    assert model.fused.last == "graph"
    rng = np.random.default_rng(5)
    p2 = dict(p)
    for k in ("embedding", "dense0/kernel", "dense0/bias", "interaction0/dense1/kernel"):
        p2[k] = (p[k] + rng.uniform(-0.05, 0.05, size=p[k].shape)).astype(np.float32)
    model.set_weights(list(p2.values()))            # in place: the captured graph is replayed on re-filled tables
    new = model(x)
    assert model.fused.last == "graph"
    fresh = _model(p2)(x)
    torch.cuda.synchronize()
    assert not torch.equal(new, old)
    assert torch.equal(new, fresh)
    assert_rows_close(new.cpu().numpy(), _oracle(p2, b), what="forward after a weight update")
    model.fused.mode = "eager"                      # unchanged weights: no table rebuild, eight launches
    before = _ffi.launch_count()
    eager = model(x)
    assert _ffi.launch_count() - before == 8
    torch.cuda.synchronize()
    assert torch.equal(eager, new)
    model.fused.check_flags()
