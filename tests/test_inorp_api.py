"""INorp without a GPU: the builder's dictionary, refusals and weight list, the route decisions, the argument checks of
the C entry points, and the identities the GPU tests rest on - the restatement (tests/inorp_reference.py) against the
oracle's primitives, the fold against the reference's op sequence, the closed-form reverse against autograd (float64, to
1e-12), and the float32 restatement of every model case within half of ``parity.BAR_CAP`` of its float64 twin."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import inorp_reference as ref
from gcnn_keras_amd import _ffi, synth
from gcnn_keras_amd.layers.conv.inorp_conv import INorpEdgeStep, fused_step_supported
from gcnn_keras_amd.literature import INorp
from parity import BAR_CAP, rowwise_rel

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import kgcnn_oracle as ko  # noqa: E402

F64 = torch.float64

# kgcnn/literature/INorp.py:23-42, as data
REFERENCE_DEFAULT = {
    "name": "INorp",
    "inputs": [{"shape": (None,), "name": "node_attributes", "dtype": "float32", "ragged": True},
               {"shape": (None,), "name": "edge_attributes", "dtype": "float32", "ragged": True},
               {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True},
               {"shape": [], "name": "graph_attributes", "dtype": "float32", "ragged": False}],
    "input_embedding": {"node": {"input_dim": 95, "output_dim": 64},
                        "edge": {"input_dim": 5, "output_dim": 64},
                        "graph": {"input_dim": 100, "output_dim": 64}},
    "set2set_args": {"channels": 32, "T": 3, "pooling_method": "mean", "init_qstar": "mean"},
    "node_mlp_args": {"units": [100, 50], "use_bias": True, "activation": ["relu", "linear"]},
    "edge_mlp_args": {"units": [100, 100, 100, 100, 50], "activation": ["relu", "relu", "relu", "relu", "linear"]},
    "pooling_args": {"pooling_method": "segment_mean"},
    "depth": 3, "use_set2set": False, "verbose": 10,
    "gather_args": {},
    "output_embedding": "graph", "output_to_tensor": True,
    "output_mlp": {"use_bias": [True, True, False], "units": [25, 10, 1], "activation": ["relu", "relu", "sigmoid"]},
}


# ------------------------------------------------------------------------------------------------------ the builder
def test_default_dictionary_is_the_references():
    assert INorp.hyper_model_default == REFERENCE_DEFAULT
    assert INorp.model_default is INorp.hyper_model_default
    assert INorp.__model_version__ == "2022.11.25"
    import gcnn_keras_amd.literature as literature
    assert literature.INorp is INorp


def test_refusals():
    with pytest.raises(ValueError, match="Unsupported output embedding for mode `INorp`"):
        INorp.make_model(output_embedding="edge")
    with pytest.raises(ValueError, match="Unsupported output embedding"):
        INorp.make_model(output_embedding=None)
    with pytest.raises(ValueError, match="matching list"):  # MLPBase: a unit list and an activation list must match
        INorp.make_model(edge_mlp_args={"units": [16, 16], "activation": ["relu", "relu", "linear"]})
    m = INorp.make_model(**ref.CONFIGS["mutag"])
    with pytest.raises(ValueError, match="expects"):
        m.set_weights([np.zeros((1, 1), np.float32)])


def _shapes(m):
    """(name below the model's layer, shape) of every weight; the running number of an MLP's name is taken out."""
    return [(re.sub(r"^mlp_\d+_", "mlp_", n.split("/", 1)[1]), tuple(t.shape)) for n, t in m.weights]


def _mlp(fin, units, biases=None):
    out = []
    for k, u in enumerate(units):
        out.append(("mlp_dense_%d/kernel" % k, (fin, u)))
        if biases is None or biases[k]:
            out.append(("mlp_dense_%d/bias" % k, (u,)))
        fin = u
    return out


def test_weight_list_of_embedded_and_feature_inputs():
    m = INorp.make_model(**ref.CONFIGS["mutag"])
    want = [("embeddings", (60, 16)), ("embeddings", (4, 8)), ("embeddings", (30, 16))]
    for _ in range(3):
        want += _mlp(2 * 16 + 8, [16, 16]) + _mlp(16 + 16 + 16, [16, 16])
    want += _mlp(16, [16, 8, 1], [True, True, False])
    assert _shapes(m) == want
    assert m.fused_step_rounds == 3 and not m.use_fused_step and m.auto_graph      # served, but off by default
    assert len({id(t) for _, t in m.weights}) == len(m.weights)          # no tensor listed twice: the steps own none
    # feature inputs: no node or edge table; the first block reads 41-wide nodes, the later ones the node MLP's 32
    m = INorp.make_model(**ref.CONFIGS["esol"])
    want = [("embeddings", (32, 32))]
    for fin in (41, 32, 32):
        want += _mlp(2 * fin + 11, [32, 32]) + _mlp(fin + 32 + 32, [32, 32])
    want += _mlp(32, [32, 32, 1], [True, True, False])
    assert _shapes(m) == want and m.fused_step_rounds == 3
    # the default dictionary: five layers 100 wide, the layer sequence
    m = INorp.make_model()
    want = [("embeddings", (95, 64)), ("embeddings", (5, 64)), ("embeddings", (100, 64))]
    for fin in (64, 50, 50):
        want += _mlp(2 * fin + 64, [100, 100, 100, 100, 50]) + _mlp(fin + 50 + 64, [100, 50])
    want += _mlp(50, [25, 10, 1], [True, True, False])
    assert _shapes(m) == want and m.fused_step_rounds == 0
    # Set2Set: its Dense, then its LSTM, stand between the blocks and the output MLP, which reads q* = 2 x channels
    plain = _shapes(INorp.make_model(**ref.CONFIGS["mutag"]))
    m = INorp.make_model(**dict(ref.CONFIGS["mutag"], use_set2set=True))
    got, lstm = _shapes(m), len(m.layers[-2].weights)
    assert lstm > 0 and len(got) == len(plain) + 2 + lstm
    assert got[:len(plain) - 5] == plain[:-5]
    assert got[len(plain) - 5:len(plain) - 3] == [("kernel", (16, 32)), ("bias", (32,))]
    assert got[-5:] == _mlp(64, [16, 8, 1], [True, True, False])
    m = INorp.make_model(**dict(ref.CONFIGS["mutag"], output_embedding="node"))
    assert _shapes(m)[-5:] == _mlp(16, [16, 8, 1], [True, True, False])


def test_switch_is_part_of_the_model():
    m = INorp.make_model(**ref.CONFIGS["esol"])
    assert all(lay.fused_step and not lay.use_fused_step for lay in m.step_layers)     # off by default
    m.use_fused_step = True
    assert m.use_fused_step and all(lay.use_fused_step for lay in m.step_layers)
    m.step_layers[1].use_fused_step = False
    assert not m.use_fused_step
    m.use_fused_step = False
    assert not m.use_fused_step and not any(lay.use_fused_step for lay in m.step_layers)
    step = m.step_layers[0]
    assert step.weight_gradients and step.weights and [n for n, _ in step._weights] == []     # no weight of its own


def test_route_decisions():
    ok = dict(node_width=41, edge_width=11, units=[32, 32], activation=["relu", "linear"], use_bias=[True, True],
              pooling_method="segment_sum")
    assert fused_step_supported(**ok)
    for h1 in (16, 32, 64, 128):
        assert fused_step_supported(**dict(ok, units=[h1, 4]))
    for name in ref.ACTIVATIONS:
        assert fused_step_supported(**dict(ok, activation=[name, "linear"]))
    for change in (dict(units=[100, 32]), dict(units=[48, 32]), dict(units=[256, 32]),         # H1 outside the four
                   dict(units=[32, 30]), dict(units=[32, 132]), dict(units=[32, 0]),            # H2
                   dict(units=[32, 32, 32], activation=["relu", "relu", "linear"], use_bias=[True] * 3),
                   dict(units=[32], activation=["linear"], use_bias=[True]),
                   dict(activation=["relu", "relu"]), dict(activation=["elu", "linear"]),
                   dict(activation=["softmax", "linear"]),
                   dict(use_bias=[True, False]), dict(use_bias=[False, True]),
                   dict(pooling_method="segment_max"), dict(pooling_method="max"), dict(pooling_index=1),
                   dict(edge_width=65), dict(edge_width=0), dict(edge_width=None), dict(node_width=None),
                   dict(dtype="float64"), dict(dtype=torch.float64), dict(plain=False)):
        assert not fused_step_supported(**dict(ok, **change)), change
    assert fused_step_supported(**dict(ok, use_bias=[False, False]))
    assert fused_step_supported(**dict(ok, edge_width=1)) and fused_step_supported(**dict(ok, edge_width=64))
    assert fused_step_supported(**dict(ok, node_width=3, pooling_method="mean", activation=["relu", None]))
    # the layer decides in build()
    lay = INorpEdgeStep(edge_mlp_args={"units": [64, 32], "activation": ["swish", "linear"]},
                        pooling_args={"pooling_method": "sum"})
    assert lay.fused_step is None
    lay.ensure_built([(None, None, 7), (None, None, 5), (None, None, 2)])
    assert lay.fused_step is True and tuple(lay.lay_mlp.mlp_dense_layer_list[0].kernel.shape) == (19, 64)
    lay = INorpEdgeStep(edge_mlp_args={"units": [64, 32], "activation": ["swish", "linear"], "use_normalization": True,
                                       "normalization_technique": "graph_layer"})
    lay.ensure_built([(None, None, 7), (None, None, 5), (None, None, 2)])
    assert lay.fused_step is False
    lay = INorpEdgeStep(edge_mlp_args={"units": [64, 32], "activation": ["swish", "linear"]}, dtype="float64")
    lay.ensure_built([(None, None, 7), (None, None, 5), (None, None, 2)])
    assert lay.fused_step is False


# ------------------------------------------------------------------------------------------------ the C entry points
def test_entry_points_are_declared_in_their_family_header():
    names = ["mp_inorp_edge_f32", "mp_inorp_edge_grad_f32", "mp_inorp_edge_ws_bytes"]
    assert [n for n in _ffi.declared_symbols() if n.startswith("mp_inorp")] == names
    assert _ffi.PENDING_HEADERS == ("mpengine/inorp.h",) and sorted(_ffi._PENDING_SIGNATURES) == names
    family = os.path.join(os.path.dirname(_ffi.HEADER_PATH), "mpengine", "inorp.h")
    text = open(family).read()
    assert "#ifndef MPENGINE_INORP_H" in text and '#include "core.h"' in text and all(n in text for n in names)
    assert all(n in _ffi.HEADER_TEXT for n in names)
    P, i, i64, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    sig = _ffi._PENDING_SIGNATURES
    assert sig["mp_inorp_edge_ws_bytes"] == [i64, i, P]
    assert sig["mp_inorp_edge_f32"] == [P, P, i64, i, P, i, P, P, i64, P, P, i, f, i, P, ctypes.c_size_t, P, P]
    assert sig["mp_inorp_edge_grad_f32"] == [P, P, i64, i, P, i, P, P, i64, P, P, i, f, i, P, P, ctypes.c_size_t, P, P, P]
    lib = _ffi.lib()
    assert lib.mp_inorp_edge_f32.argtypes == sig["mp_inorp_edge_f32"] and lib.mp_inorp_edge_f32.restype is ctypes.c_int


def _fwd_args(n=4, h1=32, fe=8, e=0, act=1, op=None, ws_bytes=0):
    return [None, None, n, h1, None, fe, None, None, e, None, None, act, 0.05, _ffi.MP_SUM if op is None else op, None,
            ws_bytes, None, None]


def _grad_args(**kw):
    a = _fwd_args(**kw)
    return a[:14] + [None] + a[14:16] + [None, None, None]


@pytest.mark.parametrize("name, args", [("mp_inorp_edge_f32", _fwd_args), ("mp_inorp_edge_grad_f32", _grad_args)])
def test_argument_checks(name, args):
    lib = _ffi.lib()
    fn = getattr(lib, name)
    for bad, word in ((dict(h1=100), b"hidden width"), (dict(h1=48), b"hidden width"), (dict(h1=0), b"hidden width"),
                      (dict(fe=0), b"edge width"), (dict(fe=65), b"edge width"),
                      (dict(act=-1), b"activation"), (dict(act=_ffi.MP_ACT_LAST + 1), b"activation"),
                      (dict(op=_ffi.MP_MAX), b"pooling"), (dict(op=17), b"pooling"),
                      (dict(n=-1), b"sizes"), (dict(n=2 ** 31 - 1), b"sizes"), (dict(e=-1), b"sizes"),
                      (dict(e=2 ** 31 - 32), b"sizes")):
        assert fn(*args(**bad)) == _ffi.MP_EINVAL, bad
        message = lib.mp_last_error()
        assert name.encode() in message and word in message, (bad, message)
    assert fn(*args(n=0)) == _ffi.MP_OK                                      # no nodes: nothing to do, no device
    assert fn(*args(n=0, e=0)) == _ffi.MP_OK
    assert fn(*args(n=4)) == _ffi.MP_EINVAL and b"null pointer" in lib.mp_last_error()
    # a short workspace is refused before anything is launched (the pointers are never followed)
    one = ctypes.c_void_p(16)
    a = args(n=4, e=40, ws_bytes=8)
    for k in range(len(a)):
        if a[k] is None:
            a[k] = one
    a[-1] = None                                                             # the stream
    assert fn(*a) == _ffi.MP_EINVAL
    message = lib.mp_last_error()
    assert name.encode() in message and b"workspace of 8 bytes, need 512" in message
    with pytest.raises(ValueError, match=name):
        _ffi.call(name, *args(h1=100))


def test_workspace_query():
    for e, h1, want in ((0, 16, 0), (1, 16, 128), (32, 32, 256), (33, 32, 512), (65, 128, 3 * 2 * 128 * 4)):
        assert _ffi.workspace_bytes("mp_inorp_edge_ws_bytes", e, h1) == want
    with pytest.raises(ValueError, match="mp_inorp_edge_ws_bytes"):
        _ffi.workspace_bytes("mp_inorp_edge_ws_bytes", 4, 100)
    with pytest.raises(ValueError, match="mp_inorp_edge_ws_bytes"):
        _ffi.workspace_bytes("mp_inorp_edge_ws_bytes", -1, 32)


# ------------------------------------------------------------------------------------------- float64 identities
def _step64(kind, node_width, edge_width, h1, h2, use_bias=True):
    b = ref.edge_list(kind)
    op = ref.step_operands(b, node_width, edge_width, h1, h2, use_bias=use_bias)
    t = {k: (None if v is None else torch.tensor(v, dtype=F64)) for k, v in op.items()}
    return b, op, t, ref.flat_indices(b)


@pytest.mark.parametrize("method", ["segment_sum", "segment_mean"])
@pytest.mark.parametrize("kind", ref.EDGE_LISTS)
def test_restatement_forms_agree(kind, method):
    """Per-edge loop = tensor form = oracle primitives = folded form, with and without bias, for two activations."""
    for activation, use_bias, (fn, fe, h1, h2) in (("relu", True, (5, 3, 16, 8)), ("swish", False, (3, 11, 32, 12))):
        b, op, t, (recv, send) = _step64(kind, fn, fe, h1, h2, use_bias)
        layers = [(t["w1"], t["b1"], activation), (t["w2"], t["b2"], "linear")]
        loop = ref.round_loop(t["nodes"], t["edges"], recv, send, t["w1"], t["b1"], t["w2"], t["b2"], activation, method)
        tensor = ref.round_tensor(t["nodes"], t["edges"], recv, send, layers, method)
        folded = ref.round_folded(t["nodes"], t["edges"], recv, send, t["w1"], t["b1"], t["w2"], t["b2"], activation,
                                  method)
        f64 = lambda a: None if a is None else np.asarray(a, np.float64)
        nodes = ko.R(f64(op["nodes"]), b["node_splits"])
        edges = ko.R(f64(op["edges"]), b["edge_splits"])
        idx = ko.R(b["edge_indices"], b["edge_splits"])
        eu = ko.lazy_concatenate([ko.lazy_concatenate([ko.gather_nodes_outgoing(nodes, idx),
                                                       ko.gather_nodes_ingoing(nodes, idx)]), edges])
        eu = ko.mlp(eu, [(f64(op["w1"]), f64(op["b1"]), activation),
                         (f64(op["w2"]), f64(op["b2"]), "linear")])
        oracle = ko.pooling_local_edges(nodes, eu, idx, pooling_method=method).values
        assert tuple(tensor.shape) == (int(b["node_splits"][-1]), h2)
        for name, other in (("loop", loop.numpy()), ("oracle", oracle), ("folded", folded.numpy())):
            assert np.max(np.abs(other - tensor.numpy()), initial=0.0) <= 1e-12, (name, kind)
        received = np.zeros(len(tensor), bool)
        received[recv.numpy()] = True
        assert not tensor.numpy()[~received].any() and not folded.numpy()[~received].any()   # exactly 0 without edges


@pytest.mark.parametrize("method", ["segment_sum", "segment_mean"])
@pytest.mark.parametrize("activation", ref.ACTIVATIONS)
def test_closed_form_reverse_against_autograd(activation, method):
    for kind in ("e33", "star70", "batch8_shuffled"):
        b, op, t, (recv, send) = _step64(kind, 5, 3, 16, 8)
        pj, pi, wc = ref.split_first(t["nodes"], t["edges"], t["w1"], t["b1"])
        leaves = [x.detach().clone().requires_grad_(True) for x in (pj, pi, t["edges"], wc)]
        out = ref.edge_kernel(leaves[0], leaves[1], leaves[2], leaves[3], recv, send, activation, method)
        g = torch.tensor(np.random.default_rng(3).normal(size=tuple(out.shape)), dtype=F64)
        pj_bar, pi_bar, e_bar, wc_bar = torch.autograd.grad(out, leaves, grad_outputs=g)
        gz, c_pi, c_pj, c_wc, c_e = ref.edge_kernel_reverse(pj, pi, t["edges"], wc, recv, send, activation, method, g)
        for name, a, c in (("Pi_bar", pi_bar, c_pi), ("Pj_bar", pj_bar, c_pj), ("Wc_bar", wc_bar, c_wc),
                           ("edges_bar", e_bar, c_e)):
            assert float((a - c).abs().max()) <= 1e-12, (name, kind)
        assert tuple(gz.shape) == (len(recv), 16)


def test_relu_derivative_at_an_exact_zero():
    z = torch.tensor([-1.0, 0.0, 2.0], dtype=F64)
    assert ref.act_grad("relu", z).tolist() == [0.0, 0.0, 1.0]


# ----------------------------------------------------------------------------- the float32 restatement's own distance
def _vec(a):
    a = np.asarray(a)
    return a.reshape(1, -1) if a.ndim == 1 else a


MODEL_CASES = [("esol", {}), ("mutag", {}), ("default", {}), ("mutag", {"output_embedding": "node"})]


@pytest.mark.parametrize("name, extra", MODEL_CASES, ids=lambda v: v if isinstance(v, str) else "-".join(v.values()))
def test_float32_restatement_is_within_half_the_cap_of_float64(name, extra):
    """The weight draws of the GPU tests: outputs and every weight gradient of the MAE loss (a bias gradient as one row),
    float32 against float64, inside ``BAR_CAP / 2``; the fold changes nothing beyond rounding; the MAE targets lie away
    from the outputs."""
    cfg = ref.spec_of(INorp, name, **extra)
    m = INorp.make_model(**dict(ref.CONFIGS[name], **extra))
    ws = ref.parity_weights(m, ref.WEIGHT_SEED[name])
    b = ref.model_batch(synth, name)
    o32, o64 = (ref.forward(ws, b, dt, cfg).numpy() for dt in (torch.float32, F64))
    rows = int(b["node_splits"][-1]) if extra else ref.GRAPHS
    assert o64.shape == (rows, 1) and float(np.abs(o64).max()) > 0.05
    print("[inorp] %s %s: float32 restatement %.2e from float64" % (name, extra, rowwise_rel(o32, o64)))
    assert rowwise_rel(o32, o64) <= BAR_CAP / 2
    unfolded = ref.forward(ws, b, F64, cfg, folded=False).numpy()
    assert np.max(np.abs(unfolded - o64)) <= 1e-12
    if extra:
        return
    target = ref.train_target(ref.GRAPHS)
    assert float(np.min(np.abs(o64 - target))) > 0.5
    (l32, g32), (l64, g64) = (ref.weight_gradients(ws, b, dt, cfg, target) for dt in (torch.float32, F64))
    assert abs(l32 - l64) <= 1e-6 * abs(l64)
    for (wname, _), a, c in zip(m.weights, g32, g64):
        assert float(c.abs().max()) > 0, wname
        err = rowwise_rel(_vec(a.numpy()), _vec(c.numpy()))
        assert err <= BAR_CAP / 2, "%s: gradient of %s: float32 %.3g from float64" % (name, wname, err)
