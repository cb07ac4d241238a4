"""HamNet on the engine: defaults, configs, weight names and order, the configuration rules of the fused routes, refusals
and the new ABI symbols.  Also pins the restatement the GPU tests measure against to a per-edge / per-graph NumPy loop.
Runs without a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import hamnet_reference as href
from gcnn_keras_amd import _ffi, _header
from gcnn_keras_amd.layers.conv import hamnet_conv as hc
from gcnn_keras_amd.layers.conv.mpnn_conv import GRUUpdate
from gcnn_keras_amd.literature import HamNet

F64 = torch.float64
NEW_SYMBOLS = ("mp_hamnet_edge_f32", "mp_hamnet_attend_f32", "mp_hamnet_fingerprint_f32")
BASE_KEYS = {"name", "trainable", "dtype", "node_indexing", "ragged_validate", "is_sorted", "has_unconnected"}
KERNEL_KEYS = {"kernel_regularizer", "activity_regularizer", "bias_regularizer", "kernel_constraint", "bias_constraint",
               "kernel_initializer", "bias_initializer"}
DROP_KEYS = {"rate", "noise_shape", "seed"}
GRU_KEYS = {"recurrent_activation", "recurrent_initializer", "recurrent_regularizer", "recurrent_constraint", "dropout",
            "recurrent_dropout", "reset_after"}


def test_hyper_model_default_is_the_references():
    # a literal copy of the values of kgcnn/literature/HamNet.py:29-47
    assert HamNet.hyper_model_default == {
        "name": "HamNet",
        "inputs": [{"shape": (None,), "name": "node_attributes", "dtype": "float32", "ragged": True},
                   {"shape": (None,), "name": "edge_attributes", "dtype": "float32", "ragged": True},
                   {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True},
                   {"shape": (None, 3), "name": "node_coordinates", "dtype": "float32", "ragged": True}],
        "input_embedding": {"node": {"input_dim": 95, "output_dim": 64}, "edge": {"input_dim": 5, "output_dim": 64}},
        "message_kwargs": {"units": 128, "units_edge": 128},
        "fingerprint_kwargs": {"units": 128, "units_attend": 128, "depth": 2},
        "gru_kwargs": {"units": 128},
        "verbose": 10, "depth": 1,
        "union_type_node": "gru",
        "union_type_edge": "None",
        "given_coordinates": True,
        "output_embedding": "graph", "output_to_tensor": True,
        "output_mlp": {"use_bias": [True, True, False], "units": [25, 10, 1], "activation": ["relu", "relu", "linear"]},
    }
    assert HamNet.__model_version__ == "2022.11.25"


def test_abi_declares_the_new_entry_points():
    family = os.path.join(os.path.dirname(_ffi.HEADER_PATH), "mpengine", "hamnet.h")   # one family under the umbrella
    core = _header.parse(_header.expand(os.path.join(os.path.dirname(family), "core.h"))).signatures
    declared = _header.parse(_header.expand(family)).signatures          # hamnet.h includes core.h, nothing else
    assert sorted(set(declared) - set(core)) == sorted(NEW_SYMBOLS)
    assert set(NEW_SYMBOLS) <= set(_ffi.declared_symbols())
    lib = _ffi.lib()
    assert all(hasattr(lib, name) for name in NEW_SYMBOLS)
    assert all(getattr(lib, name).argtypes for name in NEW_SYMBOLS)
    assert lib.mp_hamnet_attend_f32.argtypes == [ctypes.c_int] + [ctypes.c_void_p] * 2 + [ctypes.c_int64, ctypes.c_void_p,
                                                                  ctypes.c_int64] + [ctypes.c_void_p] * 2 + \
        [ctypes.c_int, ctypes.c_float] + [ctypes.c_void_p] * 2
    assert (_ffi.MP_HAMNET_MAX_DEPTH, _ffi.MP_HAMNET_MAX_WIDTH, _ffi.MP_HAMNET_MAX_COORDS) == (8, 256, 8)


# ------------------------------------------------------------------------------------------------ configs
def _round_trip(layer):
    config = layer.get_config()
    again = type(layer).from_config(config).get_config()
    assert again == config
    return set(config)


def test_gru_union_is_gru_update():
    assert hc.HamNetGRUUnion is GRUUpdate
    _round_trip(hc.HamNetGRUUnion(units=8, name="u"))


def test_naive_union_config():
    keys = _round_trip(hc.HamNetNaiveUnion(units=8, activation="relu", use_bias=False, name="n"))
    assert keys == BASE_KEYS | KERNEL_KEYS | {"units", "use_bias", "activation"}
    assert hc.HamNetNaiveUnion(units=8).get_config()["activation"] == "kgcnn>leaky_relu"


@pytest.mark.parametrize("use_dropout", [False, True])
def test_readout_attend_config(use_dropout):
    layer = hc.HamNetGlobalReadoutAttend(units=8, use_dropout=use_dropout, rate=0.2 if use_dropout else None, seed=3, name="r")
    keys = _round_trip(layer)
    assert keys == BASE_KEYS | KERNEL_KEYS | {"units", "use_bias", "use_dropout", "activation", "activation_last"} | (
        DROP_KEYS if use_dropout else set())
    config = layer.get_config()
    assert (config["activation"], config["activation_last"]) == ("kgcnn>leaky_relu", "elu")
    assert [name for name in ("gather_state", "dense_attend", "dense_align", "lay_concat", "pool_attention", "final_activ")
            if not hasattr(layer, name)] == []
    assert hasattr(layer, "dropout_layer") == use_dropout


@pytest.mark.parametrize("depth", [0, 3])
def test_fingerprint_config(depth):
    layer = hc.HamNetFingerprintGenerator(units=8, units_attend=12, depth=depth, pooling_method="sum", name="f")
    keys = _round_trip(layer)
    # the reference's keys (hamnet_conv.py:370-388); rate / noise_shape / seed are held with and without dropout
    assert keys == BASE_KEYS | KERNEL_KEYS | GRU_KEYS | DROP_KEYS | {"units", "units_attend", "use_bias", "use_dropout",
                                                                    "depth", "pooling_method", "activation"}
    assert len(layer.readouts) == len(layer.unions) == depth
    assert all(isinstance(r, hc.HamNetGlobalReadoutAttend) for r in layer.readouts)
    assert [name for name in ("pool_nodes", "vertex2mol", "final_activ") if not hasattr(layer, name)] == []
    assert layer.get_config()["depth"] == depth and layer.get_config()["pooling_method"] == "sum"


@pytest.mark.parametrize("use_dropout", [False, True])
def test_message_config(use_dropout):
    layer = hc.HamNaiveDynMessage(units=8, units_edge=12, use_dropout=use_dropout, rate=0.1 if use_dropout else None, name="m")
    keys = _round_trip(layer)
    # the reference's keys (hamnet_conv.py:530-544) and units_edge, without which the configuration cannot be rebuilt
    assert keys == BASE_KEYS | KERNEL_KEYS | {"units", "units_edge", "use_bias", "use_dropout", "activation",
                                              "activation_last"} | (DROP_KEYS if use_dropout else set())
    names = ("gather_v", "gather_p", "gather_q", "lazy_sub_p", "lazy_sub_q", "lay_concat_align", "lay_concat_edge",
             "dense_attend", "dense_align", "dense_e", "pool_attention", "final_activ")
    assert [name for name in names if not hasattr(layer, name)] == []
    assert layer.use_fused_hamnet is True and layer.return_edge_update is True


def test_the_cell_restrictions():
    for bad in (dict(reset_after=False), dict(dropout=0.1), dict(recurrent_dropout=0.1)):
        with pytest.raises(NotImplementedError):
            hc.HamNetFingerprintGenerator(units=8, units_attend=8, **bad)
    hc.HamNetFingerprintGenerator(units=8, units_attend=8, reset_after=True, dropout=0.0, recurrent_dropout=0.0)


# ------------------------------------------------------------------------------------------------ weights
def _suffixes(model):
    return [(name.split("/", 1)[1] if "/" in name else name, tuple(t.shape)) for name, t in model.weights]


def test_default_model_weight_names_shapes_and_order():
    model = HamNet.make_model()
    got = [(name.rsplit("/", 2)[-2:] if name.count("/") >= 2 else name.split("/"), tuple(t.shape))
           for name, t in model.weights]
    kinds = [(parts[-1], shape) for parts, shape in got]
    gru = [("kernel", (128, 384)), ("recurrent_kernel", (128, 384)), ("bias", (2, 384))]
    dense = lambda fin, fout: [("kernel", (fin, fout)), ("bias", (fout,))]
    want = [("embeddings", (95, 64)), ("embeddings", (5, 64))] + dense(64, 128) + dense(64, 128)
    want += dense(128, 128) + dense(6 + 128, 1) + dense(128 + 6 + 128, 128)          # attend, align, edge update
    want += gru                                                                        # node union
    want += dense(128, 128)                                                            # vertex2mol
    for _ in range(2):
        want += dense(128, 128) + dense(256, 1) + gru                                  # readout i, cell i
    want += dense(128, 25) + dense(25, 10) + [("kernel", (10, 1))]
    assert kinds == want
    names = [name for name, _ in model.weights]
    assert len(set(names)) == len(names)                                               # every weight has its own name
    message = model.message_layers[0]
    assert [n.split("/")[-1] for n, _ in message.weights] == ["kernel", "bias"] * 3
    assert [tuple(t.shape) for _, t in message.weights][::2] == [(128, 128), (134, 1), (262, 128)]
    cells = [n for n in names if "gru_cell" in n and "generator" in n]
    assert [n.split("/")[-2] for n in cells] == ["gru_cell"] * 3 + ["gru_cell_1"] * 3
    assert model.fused_hamnet_blocks == [True, True] and model.use_fused_hamnet is True
    assert model.message_layers[-1].return_edge_update is False
    assert len(href.model_params(np.random.default_rng(0), 64, 64)) == len(names)


@pytest.mark.parametrize("union_node", ["gru", "naive", "None"])
@pytest.mark.parametrize("union_edge", ["gru", "naive", "None"])
def test_union_types_build_the_restatements_parameter_list(union_node, union_edge):
    model = HamNet.make_model(depth=2, union_type_node=union_node, union_type_edge=union_edge)
    p = href.model_params(np.random.default_rng(0), 64, 64, depth=2, union_node=union_node, union_edge=union_edge)
    assert [tuple(t.shape) for _, t in model.weights] == [tuple(v.shape) for v in p.values()]
    assert [m.return_edge_update for m in model.message_layers] == [True, False]


def test_make_model_refusals():
    with pytest.raises(NotImplementedError, match="Hamiltonian engine not yet implemented"):
        HamNet.make_model(given_coordinates=False)
    with pytest.raises(ValueError, match="Unsupported output embedding"):
        HamNet.make_model(output_embedding="edge")
    with pytest.raises(ValueError, match="not in default arguments"):
        HamNet.make_model(depthato=2)
    node = HamNet.make_model(output_embedding="node")
    assert node.fingerprint is None and node.fused_hamnet_blocks == [True]


# ------------------------------------------------------------------------------------------------ configuration rules
@pytest.mark.parametrize("width,ok", [(0, False), (4, True), (6, False), (256, True), (260, False)])
def test_message_predicate_at_the_width_boundaries(width, ok):
    base = dict(units=128, units_edge=128, node_width=128, edge_width=128, coord_width=3)
    assert hc.fused_hamnet_message_supported(**base)
    for key in ("units", "units_edge", "node_width", "edge_width"):
        assert hc.fused_hamnet_message_supported(**dict(base, **{key: width})) is ok, key


def test_message_predicate_coordinates_index_dtype_and_activations():
    base = dict(units=128, units_edge=128, node_width=128, edge_width=128)
    assert [hc.fused_hamnet_message_supported(coord_width=c, **base) for c in (0, 1, 8, 9)] == [False, True, True, False]
    assert not hc.fused_hamnet_message_supported(coord_width=3, pooling_index=1, **base)
    assert not hc.fused_hamnet_message_supported(coord_width=3, dtype="float64", **base)
    assert not hc.fused_hamnet_message_supported(coord_width=3, activation="gelu", **base)
    assert hc.fused_hamnet_message_supported(coord_width=3, activation="tanh", activation_last="linear", **base)


@pytest.mark.parametrize("width,ok", [(0, False), (4, True), (6, False), (256, True), (260, False)])
def test_fingerprint_predicate_at_the_width_boundaries(width, ok):
    base = dict(units=128, units_attend=128, node_width=128)
    assert hc.fused_hamnet_fingerprint_supported(**base)
    for key in base:
        assert hc.fused_hamnet_fingerprint_supported(**dict(base, **{key: width})) is ok, key


def test_fingerprint_predicate_depth_pooling_and_dtype():
    base = dict(units=128, units_attend=64, node_width=12)
    assert [hc.fused_hamnet_fingerprint_supported(depth=d, **base) for d in (0, 8, 9)] == [True, True, False]
    assert [hc.fused_hamnet_fingerprint_supported(pooling_method=m, **base) for m in ("sum", "mean", "max", "nope")] == \
        [True, True, False, False]
    assert not hc.fused_hamnet_fingerprint_supported(dtype="float64", **base)
    assert not hc.fused_hamnet_fingerprint_supported(recurrent_activation="hard_sigmoid", **base)


def test_layers_report_what_the_predicates_say():
    message = hc.HamNaiveDynMessage(units=36, units_edge=20)
    assert message.fused_supported(12, 12, 3) and not message.fused_supported(12, 10, 3)
    message.pool_attention.pooling_index = 1
    assert not message.fused_supported(12, 12, 3)
    generator = hc.HamNetFingerprintGenerator(units=8, units_attend=20, depth=9)
    assert not generator.fused_supported(12)
    assert hc.HamNetFingerprintGenerator(units=8, units_attend=20, depth=8).fused_supported(12)


# ------------------------------------------------------------------------------------------------ restatement vs loops
def _np_act(name, x):
    if name == "kgcnn>leaky_relu":
        return np.where(x >= 0, x, 0.05 * x)
    return {"elu": lambda v: np.where(v > 0, v, np.expm1(np.minimum(v, 0.0))), "linear": lambda v: v}[name](x)


def _np_dense(x, p, name, act):
    y = x @ p[name + "/kernel"].astype(np.float64)
    if name + "/bias" in p:
        y = y + p[name + "/bias"]
    return _np_act(act, y)


def test_restated_message_equals_the_edge_loop():
    b = href.mol_batch(sizes=(5, 0, 7, 3), seed=5, fn=7, fe=4)
    rng = np.random.default_rng(6)
    p = href.message_params(rng, 7, 4, 3, 6, 5)
    h, he, q = b["x"].astype(np.float64), b["e"].astype(np.float64), b["xyz"].astype(np.float64)
    pm = rng.normal(size=q.shape)
    logits, msgs, me = [], [], []
    for (u, v), g in zip(b["flat"], he):                         # one edge at a time
        d = np.concatenate([pm[v] - pm[u], q[v] - q[u]])
        logits.append(float(_np_dense(np.concatenate([d, g]), p, "align", "linear")[0]))
        msgs.append(_np_dense(h[v], p, "attend", "kgcnn>leaky_relu"))
        me.append(_np_dense(np.concatenate([h[u], d, h[v]]), p, "edge", "kgcnn>leaky_relu"))
    mv = np.zeros((len(h), 6))
    for r in range(len(h)):                                      # one receiver at a time
        mine = [k for k in range(len(b["flat"])) if b["flat"][k, 0] == r]
        if mine:
            a = np.array([logits[k] for k in mine])
            w = np.exp(a - a.max())
            mv[r] = sum(wk * msgs[k] for wk, k in zip(w / w.sum(), mine))
    t = lambda a: torch.tensor(a, dtype=F64)
    got_mv, got_me, got_logits = href.message(t(h), t(he), t(pm), t(q), b["flat"], href.params_to(p, F64))
    np.testing.assert_allclose(got_logits.numpy()[:, 0], logits, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(got_me.numpy(), np.array(me), rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(got_mv.numpy(), _np_act("elu", mv), rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize("pooling,depth", [("mean", 3), ("sum", 1), ("mean", 0)])
def test_restated_fingerprint_equals_the_graph_loop(pooling, depth):
    rng = np.random.default_rng(8)
    splits = np.array([0, 0, 5, 6, 6, 19, 19], np.int64)            # empty first, interior and last
    node = rng.normal(size=(19, 8)).astype(np.float32)
    p = href.fingerprint_params(rng, 8, 6, 10, depth)
    out = href.fingerprint(torch.tensor(node, dtype=F64), splits, href.params_to(p, F64), depth, pooling).numpy()
    assert out.shape == (5, 6)                                       # the trailing empty graph is dropped
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    for g in range(5):                                               # one graph at a time
        rows = node[splits[g]:splits[g + 1]].astype(np.float64)
        m = _np_dense(rows, p, "v2m", "kgcnn>leaky_relu")
        s = m.sum(axis=0) if len(rows) else np.zeros(6)
        if pooling == "mean" and len(rows):
            s = s / len(rows)
        for i in range(depth):
            mm = np.zeros(10)
            if len(rows):
                a = np.array([_np_dense(np.concatenate([s, x]), p, "r%d/align" % i, "linear")[0] for x in rows])
                w = np.exp(a - a.max())
                mm = (w / w.sum()) @ _np_dense(rows, p, "r%d/attend" % i, "kgcnn>leaky_relu")
            mm = _np_act("elu", mm)
            mx = mm @ p["g%d/kernel" % i].astype(np.float64) + p["g%d/bias" % i][0]
            mh = s @ p["g%d/recurrent_kernel" % i].astype(np.float64) + p["g%d/bias" % i][1]
            z, r = sig(mx[:6] + mh[:6]), sig(mx[6:12] + mh[6:12])
            s = _np_act("kgcnn>leaky_relu", z * s + (1 - z) * np.tanh(mx[12:] + r * mh[12:]))
        np.testing.assert_allclose(out[g], s, rtol=1e-11, atol=1e-13)
    every = href.fingerprint(torch.tensor(node, dtype=F64), splits, href.params_to(p, F64), depth, pooling, rows=6).numpy()
    np.testing.assert_array_equal(every[:5], out)
    np.testing.assert_allclose(every[5], every[0], rtol=1e-12)      # a trailing empty graph, served like the first one
