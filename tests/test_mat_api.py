"""MAT's public surface, the configuration rule of the fused attention block, the refusals, the new ABI symbol, and the
restatement the GPU tests measure against (tests/mat_reference.py): its padded form and its per-molecule form are the
same function, which is why the engine may drop the padding.  Runs without a GPU."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import mat_reference as mref
from gcnn_keras_amd import _ffi
from gcnn_keras_amd.layers import casting
from gcnn_keras_amd.layers.conv import mat_conv
from gcnn_keras_amd.literature import MAT
from gcnn_keras_amd.ragged import RaggedTensor
from parity import rowwise_rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kgcnn/literature/MAT.py:23-49, written out
REFERENCE_DEFAULT = {
    "name": "MAT",
    "inputs": [
        {"shape": (None,), "name": "node_number", "dtype": "float32", "ragged": True},
        {"shape": (None, 3), "name": "node_coordinates", "dtype": "float32", "ragged": True},
        {"shape": (None, 1), "name": "edge_weights", "dtype": "float32", "ragged": True},
        {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True}
    ],
    "input_embedding": {"node": {"input_dim": 95, "output_dim": 64},
                        "edge": {"input_dim": 95, "output_dim": 64}},
    "use_edge_embedding": False,
    "max_atoms": None,
    "distance_matrix_kwargs": {"trafo": "exp"},
    "attention_kwargs": {"units": 8, "lambda_attention": 0.3, "lambda_distance": 0.3, "lambda_adjacency": None,
                         "dropout": 0.1, "add_identity": False},
    "feed_forward_kwargs": {"units": [32, 32, 32], "activation": ["relu", "relu", "linear"]},
    "embedding_units": 32,
    "depth": 5,
    "heads": 8,
    "merge_heads": "concat",
    "verbose": 10,
    "pooling_kwargs": {"pooling_method": "sum"},
    "output_embedding": "graph",
    "output_to_tensor": True,
    "output_mlp": {"use_bias": [True, True, True], "units": [32, 16, 1],
                   "activation": ["relu", "relu", "linear"]}
}


# ------------------------------------------------------------------------------------------------ padded == ragged
def _head_batch():
    """Molecules of 1, 2, 5 and 17 atoms and one without atoms (in the middle), bonds in both directions, every bond of
    the 5-atom molecule twice (duplicates add), a self loop on every second atom of the 17-atom one, shuffled."""
    rng = np.random.default_rng(3)
    sizes = [1, 2, 0, 5, 17]
    idx, counts = [], []
    for n in sizes:
        bonds = [(int(rng.integers(0, a)), a) for a in range(1, n)]
        e = [(a, b) for a, b in bonds] + [(b, a) for a, b in bonds]
        if n == 5:
            e = e + e
        if n == 17:
            e = e + [(a, a) for a in range(0, n, 2)]
        e = [e[i] for i in rng.permutation(len(e))]
        idx.append(np.array(e, dtype=np.int64).reshape(-1, 2))
        counts.append(len(e))
    ns = np.concatenate([[0], np.cumsum(sizes)])
    es = np.concatenate([[0], np.cumsum(counts)])
    n_total, m_total = int(ns[-1]), int(es[-1])
    return {"hn": rng.normal(size=(n_total, 7)), "xyz": rng.normal(0.0, 1.2, size=(n_total, 3)),
            "w": rng.choice([1.0, 1.5, 2.0, 3.0], size=m_total), "idx": np.concatenate(idx), "node_splits": ns,
            "edge_splits": es, "sizes": sizes}


@pytest.mark.parametrize("add_identity", [False, True])
@pytest.mark.parametrize("trafo", [None, "exp", "softmax"])
def test_padded_form_equals_the_loop_over_molecules(trafo, add_identity):
    b = _head_batch()
    dt = torch.float64
    units, la, ld, lg = 6, 0.3, 0.45, 0.25
    p = mref.params_to(mref.head_params(np.random.default_rng(4), 7, units), dt)
    hn, xyz, w = (torch.tensor(b[k], dtype=dt) for k in ("hn", "xyz", "w"))
    ns = b["node_splits"]
    g, nmax = len(ns) - 1, max(b["sizes"])
    h_p, h_mask_f = mref.pad(hn, ns, nmax)
    h_mask = h_mask_f.prod(dim=-1, keepdim=True)
    xyz_p, xyz_mask = mref.pad(xyz, ns, nmax)
    dist, _ = mref.distance_matrix(xyz_p, xyz_mask, trafo)
    adj = mref.dense_adjacency(w[:, None], b["idx"], b["edge_splits"], g, nmax)
    padded = mref.head_padded(h_p, h_mask, dist, adj, p, units, la, ld, lg, add_identity)
    loop = mref.head_loop(hn, xyz, w, b["idx"], ns, b["edge_splits"], p, units, trafo, la, ld, lg, add_identity)
    assert torch.isfinite(padded).all() and torch.isfinite(loop).all()
    for k in range(g):
        n = int(ns[k + 1] - ns[k])
        assert float((padded[k, :n] - loop[ns[k]:ns[k + 1]]).abs().max()) <= 1e-12 if n else True
        assert float(padded[k, n:].abs().max()) == 0.0 if n < nmax else True       # padded receivers are multiplied by 0
    assert float(loop.abs().max()) > 0.1


def test_masked_senders_have_weight_exactly_zero():
    """``exp(-1e7 - max)`` underflows in float32 and float64: the mask removes padded senders without a trace."""
    for dt in (torch.float32, torch.float64):
        scores = torch.tensor([[3.0, -2.0, 0.5, 0.0, 0.0]], dtype=dt)
        masked = scores + torch.tensor([[0.0, 0.0, 0.0, -1.0 / mref.EPS, -1.0 / mref.EPS]], dtype=dt)
        soft = torch.softmax(masked, dim=1)
        assert float(soft[0, 3]) == 0.0 and float(soft[0, 4]) == 0.0
        assert torch.equal(soft[:, :3], torch.softmax(scores[:, :3], dim=1))


def test_softmax_maximum_is_known_from_the_extrema_of_k():
    """max_j q k_j s = q s max_j k_j for q >= 0 and q s min_j k_j otherwise, exactly, in float32 too (the product is
    monotonic in k under rounding): what csrc/mp_mat.hip subtracts before every exponential."""
    rng = np.random.default_rng(5)
    q = rng.normal(size=(40, 9)).astype(np.float32)
    q[::5] = 0.0
    q[1::5] = np.abs(q[1::5])
    q[2::5] = -np.abs(q[2::5])
    k = rng.normal(size=(23, 9)).astype(np.float32)
    s = np.float32(np.sqrt(np.float32(8.0)))
    qs = q * s
    scores = qs[:, None, :] * k[None, :, :]
    known = qs * np.where(qs >= 0, k.max(axis=0)[None, :], k.min(axis=0)[None, :])
    assert scores.dtype == np.float32 and np.array_equal(scores.max(axis=1), known)
    assert np.all(scores - known[:, None, :] <= 0.0)
    assert (q == 0).any() and (q > 0).any() and (q < 0).any()


# ------------------------------------------------------------------------------------------------ the public surface
def test_model_default_is_the_references():
    assert MAT.model_default == REFERENCE_DEFAULT
    assert MAT.__model_version__ == "2022.11.25"
    assert list(inspect.signature(MAT.make_model).parameters) == [
        "name", "inputs", "input_embedding", "use_edge_embedding", "distance_matrix_kwargs", "attention_kwargs",
        "feed_forward_kwargs", "embedding_units", "depth", "heads", "merge_heads", "max_atoms", "verbose",
        "pooling_kwargs", "output_embedding", "output_to_tensor", "output_mlp"]


def test_layer_arguments_and_config_keys():
    head = mat_conv.MATAttentionHead()
    assert set(head.get_config()) >= {"units", "lambda_adjacency", "lambda_attention", "lambda_distance", "dropout",
                                      "add_identity"}
    assert (head.units, head.lambda_attention, head.lambda_distance, head.add_identity, head.get_config()["dropout"]) == \
        (64, 0.3, 0.3, False, None)
    assert head.lambda_adjacency == pytest.approx(0.4) and head.scale == 64 ** -0.5 and head.trafo == "exp"
    assert mat_conv.MATAttentionHead(lambda_adjacency=0.9).lambda_adjacency == 0.9
    assert mat_conv.MATDistanceMatrix().get_config()["trafo"] == "exp"
    with pytest.raises(ValueError):
        mat_conv.MATDistanceMatrix(trafo="tanh")
    assert mat_conv.MATGlobalPool().get_config()["pooling_method"] == "sum"
    assert mat_conv.MATReduceMask(axis=-1, keepdims=True).get_config()["keepdims"] is True
    assert mat_conv.MATExpandMask(axis=-1).get_config()["axis"] == -1
    cast = casting.CastEdgeIndicesToDenseAdjacency(n_max=7)
    assert {k: cast.get_config()[k] for k in ("n_max", "return_mask", "use_node_tensor")} == \
        {"n_max": 7, "return_mask": True, "use_node_tensor": True}


def test_compatibility_layers_on_host_tensors():
    """The dense utility layers are torch ops: against the restatement's own padded helpers."""
    b = _head_batch()
    ns, es = b["node_splits"], b["edge_splits"]
    g, nmax = len(ns) - 1, max(b["sizes"])
    xyz_p, xyz_mask = mref.pad(torch.tensor(b["xyz"], dtype=torch.float32), ns, nmax)
    for trafo in (None, "exp", "softmax"):
        got, got_mask = mat_conv.MATDistanceMatrix(trafo=trafo)(xyz_p, mask=xyz_mask)
        want, want_mask = mref.distance_matrix(xyz_p, xyz_mask, trafo)
        assert torch.equal(got, want) and torch.equal(got_mask, want_mask)
    rag = lambda v, s: RaggedTensor.from_numpy(np.ascontiguousarray(v), s, device="cpu")
    w = b["w"].astype(np.float32)[:, None]
    adj, mask = casting.CastEdgeIndicesToDenseAdjacency()([rag(b["hn"].astype(np.float32), ns), rag(w, es),
                                                           rag(b["idx"], es)])
    want = mref.dense_adjacency(torch.tensor(w), b["idx"], es, g, nmax)
    assert torch.equal(adj, want) and tuple(mask.shape) == (g, nmax, nmax)
    assert float(mask.max()) == 2.0                                 # the duplicated bonds
    assert torch.equal(mat_conv.MATReduceMask(axis=-1, keepdims=True)(xyz_mask), xyz_mask.prod(dim=-1, keepdim=True))
    assert tuple(mat_conv.MATExpandMask(axis=-1)(mask).shape) == (g, nmax, nmax, 1)
    assert torch.equal(mat_conv.MATGlobalPool()(xyz_p), xyz_p.sum(dim=1))


def test_weight_order_and_shapes_of_the_default_model():
    m = MAT.make_model(verbose=30)
    shapes = [tuple(t.shape) for _, t in m.weights]
    block = [(32,), (32,)] + [(32, 8), (8,)] * 24 + [(64, 32)] + [(32,), (32,)] + [(32, 32), (32,)] * 3 + [(32, 32)]
    want = [(95, 64), (64, 32), (1, 1)] + block * 5 + [(32,), (32,)] + [(32, 32), (32,), (32, 16), (16,), (16, 1), (1,)]
    assert shapes == want
    names = [n for n, _ in m.weights]
    assert names[0].endswith("embeddings") and names[3].endswith("gamma") and names[4].endswith("beta")
    assert all(n.endswith("bias") for n in names[6:53:2]) and all(n.endswith("kernel") for n in names[5:53:2])
    p = mref.model_params(np.random.default_rng(0), mref.config())
    assert [tuple(v.shape) for v in p.values()] == want                # the restatement's dictionary is in this order
    summed = MAT.make_model(verbose=30, merge_heads="sum", depth=1)
    assert tuple(dict(summed.weights)[[n for n, _ in summed.weights][53]].shape) == (8, 32)


def test_fused_blocks_switch_and_served_sizes():
    s = mat_conv.FUSED_MAT_SIZES
    assert s == {"units_multiple": 4, "max_channels": _ffi.MP_MAT_EPILOGUE_MAX_CHANNELS,
                 "max_width": _ffi.MP_MAT_EPILOGUE_MAX_WIDTH, "receiver_tile": _ffi.MP_MAT_RECV_TILE,
                 "sender_tile": _ffi.MP_MAT_SEND_TILE}
    ok = mat_conv.fused_mat_supported
    assert ok(8, 8, 32) and ok(4, 64, 256) and ok(32, 4, 32)
    assert not ok(6, 3, 32) and not ok(8, 33, 32) and not ok(8, 8, 257) and not ok(8, 8, 32, dtype="float64")
    m = MAT.make_model(verbose=30)
    assert m.fused_attention_blocks == [True] * 5 and m.use_fused_attention is True and m.auto_graph is True
    assert len(m.attention_heads) == 40 and len(m.attention_blocks) == 5
    m.use_fused_attention = False
    assert m.use_fused_attention is False and not any(h.use_fused_attention for h in m.attention_heads)
    assert not any(blk.supported() for blk in m.attention_blocks)
    m.use_fused_attention = True
    assert all(blk.supported() for blk in m.attention_blocks)
    small = MAT.make_model(**mref.model_kwargs(mref.model_cases()["layers-only"]))
    assert small.fused_attention_blocks == [False, False]
    # heads that differ in an argument cannot share a launch
    m.attention_heads[1].lambda_distance = 0.5
    assert not m.attention_blocks[0].supported() and m.attention_blocks[1].supported()
    soft = MAT.make_model(verbose=30, distance_matrix_kwargs={"trafo": "softmax"}, depth=1)
    assert all(h.trafo == "softmax" for h in soft.attention_heads)


def test_synthetic_batch_and_parameters():
    from gcnn_keras_amd import synth
    b = synth.mat_batch(9, seed=5)
    ns, es = b["node_splits"], b["edge_splits"]
    n, m = int(ns[-1]), int(es[-1])
    assert b["node_coordinates"].shape == (n, 3) and b["node_coordinates"].dtype == np.float32
    assert b["edge_weights"].shape == (m, 1) and set(np.unique(b["edge_weights"])) <= {1.0, 1.5, 2.0, 3.0}
    assert b["node_number"].dtype == np.float32 and b["edge_indices"].shape == (m, 2)
    for g in range(9):
        xyz = b["node_coordinates"][ns[g]:ns[g + 1]].astype(np.float64)
        d = np.linalg.norm(xyz[:, None] - xyz[None, :], axis=-1) + 10.0 * np.eye(len(xyz))
        assert d.min() >= 0.9 - 1e-6
        idx, w = b["edge_indices"][es[g]:es[g + 1]], b["edge_weights"][es[g]:es[g + 1], 0]
        order = {(int(a), int(c)): float(v) for (a, c), v in zip(idx, w)}
        assert all(order[(c, a)] == v for (a, c), v in order.items())       # a bond has one order, both directions
    again = synth.mat_batch(9, seed=5)
    assert all(np.array_equal(b[k], again[k]) for k in b)
    model = MAT.make_model(verbose=30, depth=1)
    p = synth.mat_params(model, seed=1)
    assert [tuple(v.shape) for v in p.values()] == [tuple(t.shape) for _, t in model.weights]
    gammas = [v for k, v in p.items() if k.endswith("gamma")]
    assert len(gammas) == 3 and all(np.all(np.abs(v - 1.0) <= 0.1) and np.any(v != 1.0) for v in gammas)


# ------------------------------------------------------------------------------------------------ the refusals
def _host_inputs(b):
    rag = lambda v, s: RaggedTensor.from_numpy(np.ascontiguousarray(v), s, device="cpu")
    return [rag(b["node_number"], b["node_splits"]), rag(b["node_coordinates"], b["node_splits"]),
            rag(b["edge_weights"], b["edge_splits"]), rag(b["edge_indices"], b["edge_splits"])]


def test_refusals():
    inputs = [dict(d) for d in REFERENCE_DEFAULT["inputs"]]
    inputs[2] = {"shape": (None,), "name": "edge_weights", "dtype": "float32", "ragged": True}
    with pytest.raises(NotImplementedError, match="feature axis"):
        MAT.make_model(verbose=30, inputs=inputs)
    with pytest.raises(ValueError, match="pooling_method"):
        MAT.make_model(verbose=30, pooling_kwargs={"pooling_method": "mean"})
    with pytest.raises(ValueError):
        MAT.make_model(verbose=30, output_embedding="edge")
    b = mref.model_batch(4)
    largest = int(np.diff(b["node_splits"]).max())
    m = MAT.make_model(verbose=30, depth=1, max_atoms=largest - 1)
    with torch.no_grad(), pytest.raises(ValueError, match="max_atoms"):
        m(_host_inputs(b))
    for fused in (True, False):
        m = MAT.make_model(verbose=30, depth=1)
        m.use_fused_attention = fused
        m.requires_grad_(True)
        with torch.enable_grad(), pytest.raises(NotImplementedError, match="MAT"):
            m(_host_inputs(b))
    head = mat_conv.MATAttentionHead(units=4)
    with pytest.raises(NotImplementedError):
        head([torch.zeros(1, 3, 4), torch.zeros(1, 3, 3, 1), torch.zeros(1, 3, 3, 1)])


# ------------------------------------------------------------------------------------------------ the ABI
def test_new_symbol_and_constants_in_header_and_ffi():
    text = _ffi.HEADER_TEXT
    assert re.search(r"\bint mp_mat_attention_f32\s*\(", text)
    assert "mp_mat_attention_f32" in _ffi.declared_symbols()
    for name in ("MP_MAT_RECV_TILE", "MP_MAT_SEND_TILE", "MP_MAT_TRAFO_NONE", "MP_MAT_TRAFO_EXP", "MP_MAT_TRAFO_SOFTMAX",
                 "MP_MAT_MERGE_CONCAT", "MP_MAT_MERGE_SUM", "MP_MAT_EPILOGUE_MAX_CHANNELS", "MP_MAT_EPILOGUE_MAX_WIDTH"):
        found = re.search(r"#define %s (\d+)" % name, text)
        assert found and int(found.group(1)) == getattr(_ffi, name), name
    declared = re.search(r"int mp_mat_attention_f32\s*\((.*?)\);", text, flags=re.S).group(1)
    assert len(declared.split(",")) == len(_ffi._SIGNATURES["mp_mat_attention_f32"])


def test_argument_checks_without_a_device():
    lib = _ffi.lib()
    f = lib.mp_mat_attention_f32
    base = lambda **kw: [kw.get(k, d) for k, d in (
        ("q", None), ("ldq", 8), ("k", None), ("ldk", 8), ("v", None), ("ldv", 8), ("N", 0), ("H", 1), ("U", 8),
        ("xyz", None), ("splits", None), ("G", 0), ("ptr0", None), ("perm0", None), ("send", None), ("w", None), ("M", 0),
        ("trafo", 1), ("la", 0.3), ("ld", 0.3), ("lg", 0.4), ("eye", 0), ("Wm", None), ("E", 0), ("merge", 0), ("h", None),
        ("out", None), ("flags", None), ("stream", None))]
    assert f(*base()) == _ffi.MP_OK                       # N = 0, G = 0: nothing to launch
    assert f(*base(N=0, G=3)) == _ffi.MP_OK
    assert f(*base(U=0)) == _ffi.MP_EINVAL
    assert f(*base(trafo=7)) == _ffi.MP_EINVAL
    assert f(*base(ldk=7)) == _ffi.MP_EINVAL
    assert f(*base(N=4, G=1)) == _ffi.MP_EINVAL and b"null pointer" in lib.mp_last_error()
    import ctypes
    wm = ctypes.c_void_p(64)                              # never dereferenced: the caps are checked first
    assert f(*base(Wm=wm, E=32, U=6)) == _ffi.MP_EINVAL and b"epilogue" in lib.mp_last_error()
    assert f(*base(Wm=wm, E=_ffi.MP_MAT_EPILOGUE_MAX_WIDTH + 1)) == _ffi.MP_EINVAL
    assert f(*base(Wm=wm, E=32, H=33, ldq=264, ldk=264, ldv=264)) == _ffi.MP_EINVAL
    assert f(*base(Wm=wm, E=32, merge=2)) == _ffi.MP_EINVAL
    assert f(*base(Wm=wm, E=32)) == _ffi.MP_OK
    assert f(*base(h=wm)) == _ffi.MP_EINVAL


# ------------------------------------------------------------------------------------------------ the yardstick itself
@pytest.mark.parametrize("name", sorted(mref.model_cases()))
def test_float32_restatement_is_close_to_float64(name):
    """The GPU bars (parity.assert_rows_close) lean on the float32 twin: it has to sit within 5e-6 of float64 on every
    model case the GPU file runs."""
    cfg = dict(mref.model_cases()[name])
    b = mref.model_batch()
    if name == "node-output":
        cfg["max_atoms"] = int(np.diff(b["node_splits"]).max()) + 3
    p = mref.model_params(np.random.default_rng(59), cfg)
    r32 = mref.model_forward(p, cfg, b, torch.float32).numpy()
    r64 = mref.model_forward(p, cfg, b, torch.float64).numpy()
    rows = lambda a: a.reshape(-1, a.shape[-1])
    err = rowwise_rel(rows(r32), rows(r64))
    print("[mat] %s: float32 restatement %.2e from float64" % (name, err))
    assert np.all(np.isfinite(r64)) and float(np.abs(r64).max()) > 1e-3
    assert err <= 5e-6
    g = len(b["node_splits"]) - 1
    if name == "node-output":
        assert r64.shape == (g, cfg["max_atoms"], 4)
        for k in range(g):
            assert np.all(r64[k, int(b["node_splits"][k + 1] - b["node_splits"][k]):] == 0.0)
    else:
        assert r64.shape == (g, 1)


@pytest.mark.parametrize("name", sorted(mref.kernel_cases()))
def test_kernel_cases_are_finite_in_both_twins(name):
    case = mref.kernel_case(**mref.kernel_cases()[name])
    r32, r64 = mref.kernel_restate(case, torch.float32).numpy(), mref.kernel_restate(case, torch.float64).numpy()
    assert np.all(np.isfinite(r32)) and np.all(np.isfinite(r64))
    assert r64.shape == case["q"].shape
