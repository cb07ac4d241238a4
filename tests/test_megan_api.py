"""MEGAN's public surface, the configuration rule of the fused readout, the new ABI symbols' argument checks, and the
restatement the GPU tests measure against (tests/megan_reference.py).  Runs without a GPU."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import megan_reference as mref
from gcnn_keras_amd import _ffi
from gcnn_keras_amd.literature import MEGAN
from parity import BAR_CAP, rowwise_rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mp_megan_edge_importance_f32", "mp_megan_readout_f32", "mp_megan_readout_grad_f32",
               "mp_megan_edge_importance_grad_f32")

# kgcnn/literature/MEGAN.py:55-80
DEFAULTS = {"activation": "kgcnn>leaky_relu", "use_bias": True, "dropout_rate": 0.0, "use_edge_features": True,
            "input_embedding": None, "importance_units": [], "importance_channels": 2, "importance_activation": "sigmoid",
            "importance_dropout_rate": 0.0, "importance_factor": 0.0, "importance_multiplier": 10.0, "sparsity_factor": 0.0,
            "concat_heads": True, "final_units": [1], "final_dropout_rate": 0.0, "final_activation": "linear",
            "final_pooling": "sum", "regression_limits": None, "regression_reference": None, "return_importances": True}

INPUTS = [{"shape": (None, 12), "name": "node_attributes", "dtype": "float32", "ragged": True},
          {"shape": (None, 6), "name": "edge_attributes", "dtype": "float32", "ragged": True},
          {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True}]


# ------------------------------------------------------------------------------------------------ the public surface
def test_defaults_and_config_round_trip():
    assert MEGAN.__model_version__ == "2022.12.15" and MEGAN.MEGAN.__kgcnn_model_version__ == "2022.12.15"
    sig = inspect.signature(MEGAN.MEGAN.__init__).parameters
    assert list(sig)[1] == "units" and sig["units"].default is inspect.Parameter.empty
    for name, value in DEFAULTS.items():
        default = sig[name].default
        assert (list(default) if isinstance(default, tuple) else default) == value, name
    m = MEGAN.MEGAN(units=[5, 3])
    cfg = m.get_config()
    assert set(cfg) == set(DEFAULTS) | {"units"}
    assert cfg == dict(DEFAULTS, units=[5, 3])
    other = MEGAN.MEGAN(units=[7], importance_channels=3, importance_units=[4], final_units=[6, 2], concat_heads=False,
                        final_pooling="mean", regression_limits=(-1, 1), regression_reference=0.0, sparsity_factor=0.5,
                        return_importances=False, input_embedding={"node": {"input_dim": 9, "output_dim": 4}})
    again = MEGAN.MEGAN(**other.get_config())
    assert again.get_config() == other.get_config()
    assert other.doing_regression and not m.doing_regression and other.regression_width == 2
    assert hasattr(other, "embedding_nodes") and not hasattr(m, "embedding_nodes")
    assert m.auto_graph is True
    for name in ("shifted_sigmoid", "ExplanationSparsityRegularization", "make_model"):
        assert hasattr(MEGAN, name)
    assert list(inspect.signature(MEGAN.MEGAN.__call__).parameters)[1:] == ["inputs", "training", "return_importances"]
    assert inspect.signature(MEGAN.MEGAN.__call__).parameters["return_importances"].default is False
    assert callable(m.explain_importances) and callable(m.regression_augmentation)


def test_layers_follow_the_reference_as_it_executes():
    m = MEGAN.MEGAN(units=[5, 3], importance_channels=3, importance_units=[4], final_units=[6, 2], use_bias=False,
                    final_activation="sigmoid")
    for lay, u in zip(m.attention_layers, (5, 3)):
        assert (lay.units, lay.num_heads, lay.use_final_activation, lay.has_self_loops, lay.concat_heads) == \
            (u, 3, True, True, True)
    assert [(d.units, d.activation, d.use_bias) for d in m.node_importance_layers] == [(4, "relu", False),
                                                                                      (3, "linear", False)]
    # final_biases is computed (last entry False) and never used: every final Dense gets use_bias
    assert m.final_biases == [True, False]
    assert [(d.units, d.activation, d.use_bias) for d in m.final_layers] == [(6, "relu", False), (2, "sigmoid", False)]
    assert MEGAN.MEGAN(units=[5]).final_layers[0].use_bias is True
    assert (m.lay_pool_edges_in.pooling_method, m.lay_pool_edges_in.pooling_index) == ("mean", 0)
    assert (m.lay_pool_edges_out.pooling_method, m.lay_pool_edges_out.pooling_index) == ("mean", 1)


@pytest.mark.parametrize("embed", [False, True])
def test_weight_names_and_order(embed):
    kw = dict(units=[5, 3], importance_channels=2, importance_units=[4], final_units=[6, 1])
    inputs = list(INPUTS)
    if embed:
        kw["input_embedding"] = {"node": {"input_dim": 9, "output_dim": 8, "use_embedding": True}}
        inputs[0] = dict(INPUTS[0], shape=(None,))
    m = MEGAN.make_model(inputs=inputs, **kw)
    names = [n for n, _ in m.weights]
    shapes = [tuple(t.shape) for _, t in m.weights]
    fn = 8 if embed else 12
    want = [(9, 8)] if embed else []
    width = fn
    for u in (5, 3):
        for _ in range(2):   # per head: message transform, hidden logit Dense, logit Dense
            want += [(width, u), (u,), (2 * width + 6, u), (u,), (u, 1)]
        width = 2 * u
    want += [(6, 4), (4,), (4, 2), (2,)]               # the node-importance chain on the 6-wide embeddings
    want += [(12, 6), (6,), (6, 1), (1,)]              # the final layers on K x 6 columns
    assert shapes == want
    assert len(set(names)) == len(names)
    if embed:
        assert names[0].endswith("embeddings")
    leaf = [n.rsplit("/", 1)[-1] for n in names[1 if embed else 0:]]
    assert leaf[:5] == ["kernel", "bias", "kernel", "bias", "kernel"]
    cfg = mref.config([5, 3], k=2, importance_units=[4], final_units=[6, 1], embed=(9, 8) if embed else None)
    p = mref.model_params(np.random.default_rng(0), cfg, 12, 6)
    assert [tuple(v.shape) for v in p.values()] == want     # the restatement's dictionary is in model.weights order
    # a model constructed directly builds on its first call: no weights yet, the same layer list
    lazy = MEGAN.MEGAN(**kw)
    assert lazy.weights == [] and len(lazy.layers) == len(m.layers)


@pytest.mark.parametrize("final_units", [[1], [3]])
@pytest.mark.parametrize("k", [2, 6])
def test_output_shapes_of_the_restated_model(final_units, k):
    # the reference's own shape test (final_units [1] / [3], importance_channels 2 / 6), on the restatement; the engine
    # model is held to the restatement on the GPU
    cfg = mref.config([5, 3], k=k, final_units=final_units)
    b, p = mref.model_case(cfg, seed=3, num_graphs=4)
    out, ni, ei = mref.model_restate(p, cfg, b, torch.float64)
    assert out.shape == (4, final_units[-1])
    assert ni.shape == (int(b["node_splits"][-1]), k) and ei.shape == (int(b["edge_splits"][-1]), k)
    m = MEGAN.make_model(inputs=INPUTS, **mref.model_kwargs(cfg))
    assert [tuple(t.shape) for _, t in m.weights] == [tuple(v.shape) for v in p.values()]
    assert m.fused_readout is False            # 6 and 18 columns: not a multiple of 4


def test_shifted_sigmoid_and_regression_augmentation_closed_forms():
    x = np.array([-3.0, 0.0, 5.0, 7.5, 40.0])
    np.testing.assert_allclose(MEGAN.shifted_sigmoid(x), 1 / (1 + np.exp(-(x - 5))), rtol=1e-12)
    np.testing.assert_allclose(MEGAN.shifted_sigmoid(x, shift=1, multiplier=2), 1 / (1 + np.exp(-(x - 1) / 2)), rtol=1e-12)
    t = MEGAN.shifted_sigmoid(torch.tensor(x), shift=10, multiplier=1)
    np.testing.assert_allclose(t.numpy(), 1 / (1 + np.exp(-(x - 10))), rtol=1e-12)
    assert float(MEGAN.shifted_sigmoid(5.0)) == 0.5
    m = MEGAN.MEGAN(units=[5], regression_limits=(-2, 4), regression_reference=1.0, importance_multiplier=3.0)
    y = np.array([[-2.0], [1.0], [2.5], [4.0]], np.float32)
    samples, mask = m.regression_augmentation(y)
    # |y - 1| * 3 / (0.5 * 6) = |y - 1|, twice; below / above the reference (the reference itself is in neither)
    np.testing.assert_allclose(samples.numpy(), [[3, 3], [0, 0], [1.5, 1.5], [3, 3]], rtol=1e-6)
    np.testing.assert_array_equal(mask.numpy(), [[1, 0], [0, 0], [0, 1], [0, 1]])
    cfg = mref.config([5], regression_limits=(-2, 4), regression_reference=1.0, importance_multiplier=3.0)
    rs, rm = mref.regression_augmentation(torch.from_numpy(y), cfg)
    assert torch.equal(rs, samples) and torch.equal(rm, mask)
    s = MEGAN.ExplanationSparsityRegularization(factor=0.5)
    assert s.get_config()["factor"] == 0.5
    np.testing.assert_allclose(float(s(torch.tensor([[1.0, -3.0], [0.0, 2.0]]))), 0.5 * 1.5, rtol=1e-6)
    assert len(s.losses) == 1


def test_value_and_not_implemented_errors():
    with pytest.raises(ValueError, match="importance_channels=2"):
        MEGAN.MEGAN(units=[5], importance_channels=3, regression_limits=(-1, 1), regression_reference=0.0,
                    importance_factor=1.0)
    # without the explanation step, or for a classification, any K goes
    MEGAN.MEGAN(units=[5], importance_channels=3, regression_limits=(-1, 1), regression_reference=0.0)
    MEGAN.MEGAN(units=[5], importance_channels=3, importance_factor=1.0)
    with pytest.raises(TypeError):
        MEGAN.MEGAN(units=[5], no_such_argument=1)
    m = MEGAN.make_model(inputs=INPUTS, units=[5, 3])
    with pytest.raises(RuntimeError, match="compile"):
        m.train_on_batch(None, None)
    m.compile(optimizer="sgd", loss="mean_squared_error")
    with pytest.raises(NotImplementedError, match="return_importances=True"):
        m.train_on_batch(None, None)
    for kw in ({"dropout_rate": 0.1}, {"final_dropout_rate": 0.2}):
        d = MEGAN.make_model(inputs=INPUTS, units=[5, 3], return_importances=False, **kw)
        d.compile(optimizer="sgd", loss="mean_squared_error")
        with pytest.raises(NotImplementedError, match="dropout"):
            d.train_on_batch(None, None)
        with pytest.raises(NotImplementedError, match="dropout"):
            d(None, training=True)


def test_switches_and_the_served_configurations():
    from gcnn_keras_amd.autograd import MEGAN_READOUT_SIZES
    assert MEGAN_READOUT_SIZES == {"max_channels": _ffi_const("MP_MEGAN_MAX_CHANNELS"),
                                   "max_layers": _ffi_const("MP_MEGAN_MAX_LAYERS"),
                                   "max_width": _ffi_const("MP_MEGAN_MAX_WIDTH")}
    m = MEGAN.MEGAN(units=[32, 32, 32])
    assert m.use_fused_attention is True and m.use_fused_readout is True and m.fused_readout is True
    m._graphs["sentinel"] = [0, None, None]
    m.use_fused_readout = True                      # no flip: the graphs stay
    assert "sentinel" in m._graphs
    m.use_fused_readout = False                     # a flip drops them
    assert m._graphs == {} and m.use_fused_readout is False
    m._graphs["sentinel"] = [0, None, None]
    m.use_fused_attention = False
    assert m._graphs == {} and not any(lay.use_fused_attention for lay in m.attention_layers)
    assert m._switches() == (False, False, False, False)
    m.use_fused_attention = True
    m.attention_layers[1].use_fused_attention = False       # a per-layer switch is part of a graph's identity
    assert m.use_fused_attention is False and m._switches() == (True, False, True, False)
    ok = lambda width=64, **kw: MEGAN.MEGAN(**dict(dict(units=[32]), **kw)).fused_readout_supported(width)
    assert ok() and ok(4) and ok(36) and ok(512) and ok(final_pooling="mean")
    assert not ok(6) and not ok(0) and not ok(516)
    assert ok(importance_channels=1) and ok(importance_channels=8) and not ok(importance_channels=9)
    assert ok(units=[32] * 8) and not ok(units=[32] * 9)
    assert not ok(final_pooling="max") and not ok(importance_activation="tanh")
    assert not MEGAN.MEGAN(units=[32]).fused_readout_supported(64, torch.float64)
    moved = MEGAN.MEGAN(units=[32])
    moved.lay_pool_edges_in.has_unconnected = False
    assert not moved.fused_readout_supported(64)
    assert MEGAN.MEGAN(units=[5, 3]).fused_readout is False and MEGAN.MEGAN(units=[5, 4]).fused_readout is True
    assert MEGAN.MEGAN(units=[32], concat_heads=False, importance_channels=3).fused_readout is True


def _ffi_const(name):
    text = _ffi.HEADER_TEXT
    return int(re.search(r"#define %s (\d+)" % name, text).group(1))


# ------------------------------------------------------------------------------------------------ the C ABI without a GPU
def test_new_symbols_in_header_and_table():
    text = _ffi.HEADER_TEXT
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(mp_[a-z0-9_]+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _ffi.declared_symbols(), name
        assert hasattr(_ffi.lib(), name), name
    assert _ffi_const("MP_MEGAN_NODE_TILE") == mref.NODE_TILE


def test_argument_errors_and_empty_problems():
    lib = _ffi.lib()
    one = 8     # a non-null address for checks that come before any launch
    imp = lambda l=1, m=0, k=2, group=None, ei=None: lib.mp_megan_edge_importance_f32(l, group, m, k, ei, None)
    assert imp() == _ffi.MP_OK                                                     # no edges: nothing to launch
    assert imp(k=9) == _ffi.MP_EINVAL and b"mp_megan_edge_importance_f32" in lib.mp_last_error()
    assert imp(k=0) == _ffi.MP_EINVAL and imp(l=0) == _ffi.MP_EINVAL and imp(l=9) == _ffi.MP_EINVAL
    assert imp(m=3) == _ffi.MP_EINVAL                                              # edges without pointers
    # (ei, M, K, ptr0, perm0, ptr1, perm1, z, x, N, W, splits, G, pool_op, p, ni, out, stream)
    ro = lambda m=0, k=2, n=0, w=4, g=0, op=0, splits=None, out=None: lib.mp_megan_readout_f32(
        None, m, k, None, None, None, None, None, None, n, w, splits, g, op, None, None, out, None)
    assert ro() == _ffi.MP_OK                                                      # no graph
    assert ro(k=9) == _ffi.MP_EINVAL and b"mp_megan_readout_f32" in lib.mp_last_error()
    assert ro(w=6) == _ffi.MP_EINVAL and ro(w=0) == _ffi.MP_EINVAL and ro(w=516) == _ffi.MP_EINVAL
    assert ro(w=512) == _ffi.MP_OK and ro(w=36) == _ffi.MP_OK
    assert ro(op=2) == _ffi.MP_EINVAL                                              # max pooling is not served
    assert ro(g=2) == _ffi.MP_EINVAL                                               # graphs without pointers
    assert ro(g=2, n=5, splits=one, out=16) == _ffi.MP_EINVAL                      # nodes without pointers
    assert ro(n=2 ** 31) == _ffi.MP_EINVAL
    # (g_out, g_ni, x, z, p, N, K, W, splits, G, pool_op, x_bar, z_bar, q, stream)
    rg = lambda n=0, k=2, w=4, g=0, op=0: lib.mp_megan_readout_grad_f32(None, None, None, None, None, n, k, w, None, g, op,
                                                                        None, None, None, None)
    assert rg() == _ffi.MP_OK
    assert rg(k=9) == _ffi.MP_EINVAL and b"mp_megan_readout_grad_f32" in lib.mp_last_error()
    assert rg(w=6) == _ffi.MP_EINVAL and rg(op=3) == _ffi.MP_EINVAL
    assert rg(n=3, g=1) == _ffi.MP_EINVAL and rg(n=3) == _ffi.MP_EINVAL            # nodes without pointers / graphs
    # (g_ei, q, ei, cols, ptr0, ptr1, N, M, K, s_bar, stream)
    eg = lambda n=0, m=0, k=2: lib.mp_megan_edge_importance_grad_f32(None, None, None, None, None, None, n, m, k, None, None)
    assert eg() == _ffi.MP_OK and eg(n=4) == _ffi.MP_OK
    assert eg(k=9) == _ffi.MP_EINVAL and b"mp_megan_edge_importance_grad_f32" in lib.mp_last_error()
    assert eg(n=4, m=3) == _ffi.MP_EINVAL                                          # edges without pointers


# ------------------------------------------------------------------------------------------------ the GPU cases' own budget
def _rows(a):
    return a.reshape(a.shape[0], -1)


@pytest.mark.parametrize("name", sorted(mref.model_cases()) + sorted(mref.unserved_cases()))
def test_model_cases_float32_inside_half_the_cap_and_unsaturated(name):
    cfg = dict(mref.model_cases(), **mref.unserved_cases())[name]
    b, p = mref.model_case(cfg)
    r32 = [t.numpy() for t in mref.model_restate(p, cfg, b, torch.float32)]
    r64 = [t.numpy() for t in mref.model_restate(p, cfg, b, torch.float64)]
    for what, a32, a64 in zip(("out", "node importances", "edge importances"), r32, r64):
        assert np.all(np.isfinite(a64)) and a32.shape == a64.shape
        err = rowwise_rel(_rows(a32), _rows(a64))
        print("[megan] %s %s: float32 restatement %.2e from float64" % (name, what, err))
        assert err <= BAR_CAP / 2, (name, what)
    ei = r64[2]
    inside = float(np.mean((ei >= 0.02) & (ei <= 0.98)))
    print("[megan] %s: %.2f %% of the edge importances in [0.02, 0.98]; node importances %.3f..%.3f" % (
        name, 100 * inside, r64[1].min(), r64[1].max()))
    assert inside >= 0.95, name      # a sigmoid pinned at 0 or 1 would hide a wrong logit


@pytest.mark.parametrize("name", sorted(mref.kernel_cases()))
def test_kernel_cases_float32_inside_half_the_cap(name):
    case = mref.kernel_case(**mref.kernel_cases()[name])
    r32, r64 = mref.kernel_restate(case, torch.float32), mref.kernel_restate(case, torch.float64)
    for what in r64:
        err = rowwise_rel(_rows(r32[what]), _rows(r64[what]))
        assert err <= BAR_CAP / 2, (name, what, err)
    ei = r64["ei"]
    assert float(np.mean((ei >= 0.02) & (ei <= 0.98))) >= 0.95


def test_kernel_cases_have_the_shapes_they_claim():
    import topologies as topo
    cases = mref.kernel_cases()
    assert {c["k"] for c in cases.values()} == {1, 2, 8} and {c["layers"] for c in cases.values()} == {1, 3, 8}
    assert {c["w"] for c in cases.values()} == {4, 32, 36, 64, 512}
    assert {c["pooling"] for c in cases.values()} == {"sum", "mean"}
    hub = mref.kernel_case(**cases["hub-shuffled-k8-w36-l8-mean"])
    assert topo.in_degrees(hub["flat"], hub["rows"]).max() == 1000
    assert np.any(hub["flat"][:, 0] == hub["flat"][:, 1])                          # self loops
    assert len(np.unique(hub["flat"], axis=0)) < len(hub["flat"])                  # duplicate edges
    assert np.any(np.diff(hub["flat"][:, 0]) < 0)                                  # shuffled
    sizes = np.diff(hub["row_splits"])
    assert sizes[0] == 0 and sizes[-1] == 0 and 0 in sizes[1:-1] and 1 in sizes    # empty graphs, a lone node
    send = mref.kernel_case(**cases["hubsend-sorted-k8-w32-l3-sum"])
    assert topo.in_degrees(send["flat"], send["rows"], column=1).max() == 1000
    assert np.all(np.diff(send["flat"][:, 1]) >= 0) and np.any(np.diff(send["flat"][:, 0]) < 0)
    tiles = np.diff(mref.kernel_case(**cases["tiles-sorted-k2-w32-l1-mean"])["row_splits"])
    for n in (mref.NODE_TILE - 1, mref.NODE_TILE, mref.NODE_TILE + 1, 2 * mref.NODE_TILE + 3, 1, 0):
        assert n in tiles
    e = mref.directed_edges()
    deg_in, deg_out = np.bincount(e[:, 0], minlength=6), np.bincount(e[:, 1], minlength=6)
    assert deg_in[0] == 0 and deg_out[0] > 0 and deg_out[5] == 0 and deg_in[5] > 0      # only outgoing / only incoming
    assert deg_in[4] == 0 and deg_out[4] == 0 and np.any(deg_in != deg_out)
    assert list(deg_in) == [0, 3, 2, 2, 0, 3] and list(deg_out) == [3, 2, 3, 2, 0, 0]


def test_total_loss_restatement_by_hand():
    cfg = mref.config([5], regression_limits=(-1, 1), regression_reference=0.0, importance_factor=2.0, sparsity_factor=0.5,
                      importance_multiplier=1.0)
    out = torch.tensor([[0.5], [-0.25]], dtype=torch.float64)
    y = torch.tensor([[1.0], [-1.0]], dtype=torch.float64)
    ni = torch.tensor([[0.2, 0.4], [0.1, 0.3], [0.6, 0.0]], dtype=torch.float64)
    splits = np.array([0, 2, 3])
    total, exp = mref.total_loss(out, ni, y, splits, cfg, "mean_squared_error")
    mse = (0.25 + 0.5625) / 2
    sparsity = 0.5 * float(ni.mean())
    # outs = [[0.3, 0.7], [0.6, 0.0]]; samples = |y| / 1 = 1; mask = [[0, 1], [1, 0]]
    mae = (abs(0.0 - 0.0) + abs(1 - 0.7)) / 2 / 2 + (abs(1 - 0.6) + 0.0) / 2 / 2
    np.testing.assert_allclose(float(exp), 2.0 * 2 * mae, rtol=1e-12)
    np.testing.assert_allclose(float(total), mse + sparsity + 2.0 * 2 * mae, rtol=1e-12)
    cls = mref.config([5], importance_factor=1.0, importance_multiplier=0.5)
    yc = torch.tensor([[1.0, 0.0], [0.0, 1.0]], dtype=torch.float64)
    pred = torch.sigmoid(torch.tensor([[0.3, 0.7], [0.6, 0.0]], dtype=torch.float64) - 0.5)
    want = mref.keras_loss("binary_crossentropy", pred, yc)
    _, exp = mref.total_loss(torch.sigmoid(torch.zeros(2, 2, dtype=torch.float64)), ni, yc, splits, cls,
                             "binary_crossentropy")
    np.testing.assert_allclose(float(exp), float(want), rtol=1e-12)


def test_synth_batch_and_params_are_seeded():
    from gcnn_keras_amd import synth
    a, b = synth.megan_batch(num_graphs=5, seed=9), synth.megan_batch(num_graphs=5, seed=9)
    base = synth.qm9_like_batch(num_graphs=5, seed=9)
    n, m = int(base["node_splits"][-1]), int(base["edge_splits"][-1])
    assert np.array_equal(a["edge_indices"], base["edge_indices"]) and np.array_equal(a["node_splits"], base["node_splits"])
    assert a["node_attributes"].shape == (n, 12) and a["edge_attributes"].shape == (m, 6) and a["node_type"].shape == (n,)
    assert a["node_attributes"].dtype == np.float32 and a["node_type"].min() >= 0 and a["node_type"].max() < 95
    for key in ("node_attributes", "edge_attributes", "node_type"):
        assert np.array_equal(a[key], b[key])
    assert not np.array_equal(a["node_attributes"], synth.megan_batch(num_graphs=5, seed=10)["node_attributes"][:n])
    model = MEGAN.make_model(inputs=INPUTS, units=[5, 3])
    p, q = synth.megan_params(model), synth.megan_params(model)
    assert [tuple(v.shape) for v in p.values()] == [tuple(t.shape) for _, t in model.weights]
    assert all(np.array_equal(u, v) for u, v in zip(p.values(), q.values()))
    bias = [v for k, v in p.items() if k.endswith("bias")]
    assert bias and all(np.abs(v).max() <= 0.1 for v in bias)
