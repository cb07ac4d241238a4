"""DMPNN's fused round without a GPU: the closed forms of the round's reverse (what csrc/mp_dmpnn.hip and the
gathered-difference weight gradient compute) against float64 autograd of the restatement (tests/dmpnn_reference.py), the
restatement against the NumPy oracle on the draw of the GPU model test, the route decisions, the unchanged weight list, the
switch, the refusals, the new entry points of the C-ABI, and the noise floor of the float32 restatement under the test
weights."""
import numpy as np
import pytest
import torch

import dmpnn_reference as ref
from gcnn_keras_amd import _ffi, synth
from gcnn_keras_amd.layers.conv.dmpnn_conv import DMPNNStep, fused_step_supported, fused_step_tape_supported
from gcnn_keras_amd.layers.modules import Activation, Dense
from gcnn_keras_amd.literature import DMPNN
from oracle import kgcnn_oracle as ko
from parity import rowwise_rel


# ------------------------------------------------------------------------------------------------- the closed forms
def _tiny_graph():
    """4 nodes, 7 directed edges.  rev: edge 1 has none (-1), edge 2 is its own reverse, edges 3 and 4 name the same
    reverse (edge 0), which makes rev no involution; node 3 sends nothing and node 2 receives nothing."""
    recv = torch.tensor([0, 0, 1, 1, 3, 3, 0])
    send = torch.tensor([1, 2, 0, 2, 0, 1, 1])
    rev = torch.tensor([2, -1, 2, 0, 0, 6, 5])
    return recv, send, rev, 4


@pytest.mark.parametrize("edge_activation", ["relu", "linear"])
def test_closed_forms_of_the_reverse_against_float64_autograd(edge_activation):
    recv, send, rev, n = _tiny_graph()
    rng = np.random.default_rng(11)
    f, e = 6, len(recv)
    t = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)
    h, h0 = t(rng.normal(size=(e, f))), t(rng.normal(size=(e, f)))
    w, b = t(rng.normal(size=(f, f))), t(rng.normal(size=f))
    g = torch.tensor(rng.normal(size=(e, f)))
    y = ref.round_loop(h, h0, recv, send, rev, w, b, "linear", edge_activation, n=n)
    h_bar, h0_bar, w_bar, b_bar = torch.autograd.grad(y, (h, h0, w, b), grad_outputs=g)
    with torch.no_grad():
        p, q, dw, db, hb = ref.round_reverse(g, y, h, recv, send, rev, w, n, edge_activation)
    # q is the gradient of the difference, the Dense's input
    d = ref.difference(h.detach(), recv, send, rev, n).requires_grad_(True)
    z = ref.act(edge_activation, ref.dense(d, w.detach(), b.detach(), "linear") + h0.detach())
    d_bar, = torch.autograd.grad(z, d, grad_outputs=g)
    for name, got, want in (("p", p, h0_bar), ("q", q, d_bar), ("dW", dw, w_bar), ("db", db, b_bar), ("h_bar", hb, h_bar)):
        assert float(torch.max(torch.abs(got - want))) <= 1e-12, name
    if edge_activation == "relu":
        assert bool((y == 0).any()) and bool((p[y == 0] == 0).all())


def test_round_loop_and_tensor_form_agree():
    recv, send, rev, n = _tiny_graph()
    rng = np.random.default_rng(12)
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    h, h0, w, b = t(rng.normal(size=(7, 5))), t(rng.normal(size=(7, 5))), t(rng.normal(size=(5, 5))), t(rng.normal(size=5))
    for a1, a2 in (("linear", "relu"), ("relu", "swish"), ("linear", "linear")):
        loop = ref.round_loop(h, h0, recv, send, rev, w, b, a1, a2, n=n)
        step = ref.round_step(h, h0, recv, send, rev, w, b, a1, a2, n=n)
        assert float(torch.max(torch.abs(loop - step))) <= 1e-13
    b5 = synth.cmpnn_batch(3, seed=8)
    recv, send, rev = ref.flat_indices(b5)
    e = len(recv)
    h, h0 = t(rng.normal(size=(e, 5))), t(rng.normal(size=(e, 5)))
    nn = int(b5["node_splits"][-1])
    assert float(torch.max(torch.abs(ref.round_loop(h, h0, recv, send, rev, w, None, n=nn)
                                     - ref.round_step(h, h0, recv, send, rev, w, None, n=nn)))) <= 1e-13


# ------------------------------------------------------------------------------- the restatement against the oracle
def test_restatement_against_the_oracle_on_the_model_tests_draw():
    for depth in (3, 5):
        case = ref.builder_draw(synth, depth=depth)
        b, p = case["batch"], case["params"]
        es = b["edge_splits"]
        want = ko.dmpnn_forward(p, ko.R(b["node_attributes"], b["node_splits"]), ko.R(b["edge_attributes"], es),
                                ko.R(b["edge_indices"], es), ko.R(b["edge_indices_reverse"], es), depth=depth)
        got = ref.forward(case["weights"], b, torch.float32, depth=depth, embed_nodes=False, embed_edges=False).numpy()
        assert got.shape == (5, 1)
        assert np.max(np.abs(got - np.asarray(want))) <= 2e-5 * max(1.0, float(np.max(np.abs(want))))


# -------------------------------------------------------------------------------------------------- route decisions
def test_supported_decisions():
    for f in (128, 64, 4):
        assert fused_step_supported(f, f, f, "linear", "relu")
        assert fused_step_supported(f, f, f, "relu", "swish")
    assert not fused_step_supported(130, 130, 130, "linear", "relu")
    assert not fused_step_supported(2, 2, 2, "linear", "relu")
    assert not fused_step_supported(128, 64, 64, "linear", "relu")        # edge_initialize != edge_dense units
    assert not fused_step_supported(64, 64, 128, "linear", "relu")
    assert not fused_step_supported(64, 64, 64, "elu", "relu")
    assert not fused_step_supported(64, 64, 64, "linear", "relu", dtype="float64")
    assert fused_step_tape_supported("linear", "relu") and fused_step_tape_supported(None, "linear")
    assert not fused_step_tape_supported("linear", "swish") and not fused_step_tape_supported("relu", "relu")
    # the decision is taken at build
    assert DMPNN.make_model().fused_step_rounds == [True] * 5
    unit = lambda u, a="relu": {"units": u, "use_bias": True, "activation": a}
    for width in (128, 64, 4):
        m = DMPNN.make_model(edge_initialize=unit(width), edge_dense=unit(width, "linear"), depth=2)
        assert m.fused_step_rounds == [True, True] and all(lay.fused_step_tape for lay in m.step_layers)
    m = DMPNN.make_model(edge_initialize=unit(130), edge_dense=unit(130, "linear"), depth=2)
    assert m.fused_step_rounds == [False, False]
    m = DMPNN.make_model(edge_initialize=unit(128), edge_dense=unit(64, "linear"), depth=1)
    assert m.fused_step_rounds == [False]
    # swish is served forward and steps aside on a tape
    m = DMPNN.make_model(edge_activation={"activation": "swish"}, depth=2)
    assert m.fused_step_rounds == [True, True] and not any(lay.fused_step_tape for lay in m.step_layers)
    # the node pooling of the builder does not concern the directed pooling, which is always a sum
    m = DMPNN.make_model(pooling_args={"pooling_method": "mean"}, depth=2)
    assert m.fused_step_rounds == [True, True]


def test_weight_names_and_order_are_the_parents():
    model = DMPNN.make_model()
    ws = [(n, tuple(t.shape)) for n, t in model.weights]
    assert [s for _, s in ws] == [(95, 64), (5, 64), (128, 128), (128,), (128, 128), (128,), (192, 128), (128,),
                                  (128, 64), (64,), (64, 32), (32,), (32, 1)]
    assert [n.rsplit("/", 1)[-1] for n, _ in ws] == ["embeddings"] * 2 + ["kernel", "bias"] * 5 + ["kernel"]
    # one name per owning layer, no round in front of it: embeddings, the h0 Dense, the edge Dense, the node Dense, the MLP
    owners = [n.split("/", 1)[0] for n, _ in ws]
    assert owners[0].startswith("optional_input_embedding") and owners[1].startswith("optional_input_embedding")
    assert all(o.startswith("dense_embedding") for o in owners[2:8]) and len(set(owners[2:8])) == 3
    assert all(n.startswith("mlp") and n.count("/") == 2 for n, _ in ws[8:])
    assert not any("dmpnn_step" in n for n, _ in ws)
    # every round holds the ONE shared Dense
    assert len(model.step_layers) == 5 and len({id(lay.lay_dense) for lay in model.step_layers}) == 1
    assert model.step_layers[0].lay_dense.kernel is model.layers[3].kernel
    assert model.auto_graph is True and model.use_fused_step is True
    assert model.__kgcnn_model_version__ == "2022.11.25"
    assert all(t is not None for _, t in model.weights)
    model.set_weights(ref.parity_weights(model))


def test_step_config_and_defaults():
    lay = DMPNNStep(dense=Dense(units=64, activation="linear", use_bias=False), activation=Activation(activation="swish"))
    conf = lay.get_config()
    assert conf["edge_dense"]["units"] == 64 and conf["edge_dense"]["use_bias"] is False
    assert conf["edge_dense"]["activation"] == "linear" and conf["edge_activation"]["activation"] == "swish"
    twin = DMPNNStep.from_config(conf)
    assert twin.get_config()["edge_dense"]["units"] == 64
    assert twin.lay_act.activation == "swish" and twin.lay_dense.use_bias is False
    assert DMPNNStep.weight_gradients is True and lay.use_fused_step is True and lay.fused_step is None
    lay.ensure_built([(None, None, 9), (None, None, 64), (None, None, 64), (None, None, 2), (None, None, 1)])
    assert lay.fused_step is True and lay.fused_step_tape is False and tuple(lay.lay_dense.kernel.shape) == (64, 64)


def test_switch_drops_captured_graphs():
    model = DMPNN.make_model(depth=2)
    model._graphs["some inputs"] = [2, object()]
    model.use_fused_step = True                 # no change: the graphs stay
    assert len(model._graphs) == 1
    model.use_fused_step = False
    assert model._graphs == {} and model.use_fused_step is False
    assert all(not lay.use_fused_step for lay in model.step_layers)
    model._graphs["some inputs"] = [2, object()]
    model.use_fused_step = True
    assert model._graphs == {} and model.use_fused_step is True
    model.step_layers[1].use_fused_step = False  # one round switched behind the model's back
    assert model.use_fused_step is False


def test_refusals_stay():
    with pytest.raises(NotImplementedError):
        DMPNN.make_model(use_graph_state=True)
    with pytest.raises(ValueError, match="Unsupported graph embedding for mode `DMPNN`"):
        DMPNN.make_model(output_embedding="edge")
    with pytest.raises(ValueError):
        DMPNN.make_model(no_such_key=1)


# --------------------------------------------------------------------------------------------------------- the ABI
def test_new_entry_points_in_header_table_and_library():
    import os
    names = ("mp_directed_edge_update_grad_f32", "mp_directed_edge_wgrad_ws_bytes", "mp_directed_edge_wgrad_f32",
             "mp_directed_edge_hgrad_f32")
    header = _ffi.HEADER_TEXT
    lib = _ffi.lib()
    for name in names:
        assert name in _ffi.declared_symbols() and ("int %s(" % name) in header and hasattr(lib, name), name
    # argument errors and empty problems, without a device
    assert lib.mp_directed_edge_update_grad_f32(None, None, 0, 64, None, 1, None, None, None) == _ffi.MP_OK
    assert lib.mp_directed_edge_update_grad_f32(None, None, 0, 6, None, 1, None, None, None) == _ffi.MP_EINVAL
    assert lib.mp_directed_edge_update_grad_f32(None, None, 0, 64, None, 4, None, None, None) == _ffi.MP_EINVAL  # swish
    assert b"mp_directed_edge_update_grad_f32" in lib.mp_last_error()
    assert lib.mp_directed_edge_hgrad_f32(None, 0, None, 0, 64, None, None, None, None, None, None) == _ffi.MP_OK
    assert lib.mp_directed_edge_wgrad_f32(None, 0, None, 0, 6, None, None, None, None, None, None, 0, None,
                                          None) == _ffi.MP_EINVAL
    # the row split is mp_dense_wgrad_f32's: the same workspace for the same sizes
    for e, f in ((0, 64), (32, 64), (33, 64), (5000, 128), (129, 300)):
        assert _ffi.workspace_bytes("mp_directed_edge_wgrad_ws_bytes", e, f) == \
            _ffi.workspace_bytes("mp_dense_wgrad_ws_bytes", e, f, f)
    assert _ffi.workspace_bytes("mp_directed_edge_wgrad_ws_bytes", 32, 64) == 0          # a single chunk
    assert _ffi.workspace_bytes("mp_directed_edge_wgrad_ws_bytes", 129, 64) > 0          # several


# ------------------------------------------------------------------------------------- the restatement's noise floor
def test_float32_restatement_noise_floor_of_the_gpu_cases():
    """Under the test weights (Glorot x 0.5) the float32 restatement stays within 5e-6 (rowwise_rel) of its float64 twin
    on the edge states, the node Dense and the output of every model configuration the GPU tests run, on the draws they use,
    and so does every weight gradient of the training case within 2.5e-5 - the condition under which the GPU tests compare
    float32 pipelines at parity.py's default cap."""
    for depth, width in ref.MODEL_CASES:
        _, b, ws, fwd = ref.model_case(synth, DMPNN.make_model, depth, width)
        r32, r64 = (ref.forward(ws, b, dt, states=True, **fwd) for dt in (torch.float32, torch.float64))
        for key in ("h", "node_dense", "out"):
            err = rowwise_rel(r32[key].numpy(), r64[key].numpy())
            print("[noise floor] depth %d F=%d %s: %.2e" % (depth, width, key, err))
            assert err <= 5e-6, (depth, width, key, err)
    model = DMPNN.make_model(**ref.model_kwargs(64, 3, output_embedding="node"))
    b, ws = synth.cmpnn_batch(12, seed=ref.NODE_SEED[0]), ref.parity_weights(model, ref.NODE_SEED[1])
    r32, r64 = (ref.forward(ws, b, dt, depth=3, output_embedding="node").numpy() for dt in (torch.float32, torch.float64))
    assert rowwise_rel(r32, r64) <= 5e-6
    # the weight gradients of the training case
    for width in ref.TRAIN_WIDTHS:
        model = DMPNN.make_model(**ref.model_kwargs(width, 3))
        b, ws = synth.cmpnn_batch(6, seed=ref.TRAIN_SEED[0]), ref.parity_weights(model, ref.TRAIN_SEED[1])
        g32, g64 = (ref.weight_gradients(ws, b, dt, depth=3) for dt in (torch.float32, torch.float64))
        for (name, _), a, c in zip(model.weights, g32, g64):
            err = rowwise_rel(a.numpy(), c.numpy())
            print("[noise floor] gradient F=%d %s: %.2e" % (width, name, err))
            assert err <= 2.5e-5, (width, name, err)
