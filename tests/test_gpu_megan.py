"""MEGAN on csrc/mp_megan.hip: the four kernels through the C ABI, the model on both readout routes crossed with both
attention routes, graph replay, the launch counts, and training with the explanation co-training step, all against
tests/megan_reference.py (float32 and float64).  Index lists come from tests/topologies.py.

Bars: rows and gradients through ``parity.assert_rows_close`` with its default bar and ``BAR_CAP``; rows of nodes without
edges and of graphs without nodes exactly 0; two runs and a run on a second stream equal bits."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import megan_reference as mref
from gcnn_keras_amd import _ffi
from parity import assert_rows_close

pytestmark = pytest.mark.gpu

INPUTS = [{"shape": (None, mref.FN), "name": "node_attributes", "dtype": "float32", "ragged": True},
          {"shape": (None, mref.FE), "name": "edge_attributes", "dtype": "float32", "ragged": True},
          {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True}]


def _rag(values, splits):
    from gcnn_keras_amd.ragged import RaggedTensor
    return RaggedTensor.from_numpy(values, splits)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")       # every element has to be written


def _rows(a):
    return a.reshape(a.shape[0], -1)


def _grad_rows(g):
    """The rows of a weight gradient: the rows of a kernel or an embedding table; a bias vector is ONE row.  A bias
    gradient is a column sum over every node or edge row of terms of both signs, so a component that cancels to 1e-3 of
    the vector's largest carries the float32 rounding of the whole sum (about sqrt(rows) x 6e-8 of the typical term, a
    few 1e-7 of the vector's scale for 1300 edges) whoever adds it up: held as a row of its own, against ``parity``'s
    floor of 1e-3 of the scale, it would have to agree to 1e-8 of the scale, which float32 pipelines that sum in
    different orders cannot (the layer sequence's hidden logit Dense bias came out 1.31e-05 on that measure)."""
    return g.reshape(1, -1) if g.ndim == 1 else g.reshape(g.shape[0], -1)


# ------------------------------------------------------------------------------------------------ the kernels alone
@functools.lru_cache(maxsize=None)
def _kernel_case(name):
    case = mref.kernel_case(**mref.kernel_cases()[name])
    return case, mref.kernel_restate(case, torch.float32), mref.kernel_restate(case, torch.float64)


@functools.lru_cache(maxsize=None)
def _kernel_reverse(name, with_g_ni, with_g_ei):
    case = _kernel_case(name)[0]
    return (mref.kernel_restate(case, torch.float32, with_g_ni, with_g_ei),
            mref.kernel_restate(case, torch.float64, with_g_ni, with_g_ei))


def _plan(case):
    nodes = _rag(np.zeros((case["rows"], 1), np.float32), case["row_splits"])
    idx = _rag(case["indices"], case["index_splits"])
    plan = idx.index_plan(nodes)
    plan.validate()
    return plan, nodes.row_splits


def _forward(case, plan, splits, dev):
    """``(ei, p, ni, out)`` of the two forward entry points on the current stream."""
    n, m, k, w = plan.N, plan.M, case["k"], case["w"]
    g = len(case["row_splits"]) - 1
    (ptr0, perm0, _), (ptr1, perm1, _) = plan.csr(0), plan.csr(1)
    group = (ctypes.c_void_p * len(dev["logits"]))(*[t.data_ptr() for t in dev["logits"]])
    ei, p, ni, out = _nan(m, k), _nan(n, k), _nan(n, k), _nan(g, k * w)
    _ffi.call("mp_megan_edge_importance_f32", len(dev["logits"]), group, m, k, _ffi.ptr(ei), _ffi.stream())
    _ffi.call("mp_megan_readout_f32", _ffi.ptr(ei), m, k, _ffi.ptr(ptr0), _ffi.ptr(perm0), _ffi.ptr(ptr1), _ffi.ptr(perm1),
              _ffi.ptr(dev["z"]), _ffi.ptr(dev["x"]), n, w, _ffi.ptr(splits), g, _ffi.MP_MEAN if case["pooling"] == "mean"
              else _ffi.MP_SUM, _ffi.ptr(p), _ffi.ptr(ni), _ffi.ptr(out), _ffi.stream())
    return ei, p, ni, out


def _device_inputs(case):
    return {"logits": [_cuda(a) for a in case["logits"]], "z": _cuda(case["z"]), "x": _cuda(case["x"])}


@pytest.mark.parametrize("name", sorted(mref.kernel_cases()))
def test_forward_kernels_against_the_restatement(name):
    case, r32, r64 = _kernel_case(name)
    plan, splits = _plan(case)
    dev = _device_inputs(case)
    first = _forward(case, plan, splits, dev)
    again = _forward(case, plan, splits, dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _forward(case, plan, splits, dev)
    side.synchronize()
    torch.cuda.synchronize()
    for a, b, c in zip(first, again, other):
        assert torch.equal(a, b), "two runs differ"
        assert torch.equal(a, c), "a second stream differs"
    _, perm0, _ = plan.csr(0)
    _, perm1, _ = plan.csr(1)
    if "shuffled" in name:
        assert perm0 is not None and perm1 is not None
    elif name.startswith("hub-sorted"):
        assert perm0 is None and perm1 is not None
    elif name.startswith("hubsend-sorted"):
        assert perm1 is None and perm0 is not None
    got = dict(zip(("ei", "p", "ni", "out"), (t.cpu().numpy() for t in first)))
    for what in ("ei", "p", "ni", "out"):
        assert got[what].shape == r64[what].shape and np.all(np.isfinite(got[what])), what
        assert_rows_close(_rows(got[what]), _rows(r32[what]), _rows(r64[what]), what="%s %s" % (name, what))
    deg0 = np.bincount(case["flat"][:, 0], minlength=case["rows"])
    deg1 = np.bincount(case["flat"][:, 1], minlength=case["rows"])
    lonely = (deg0 == 0) & (deg1 == 0)
    assert lonely.any() and np.all(got["p"][lonely] == 0.0) and np.all(got["ni"][lonely] == 0.0)
    empty = np.diff(case["row_splits"]) == 0
    assert empty.any() and np.all(got["out"][empty] == 0.0)
    if name.startswith("directed"):
        # each list alone: a node with only outgoing edges gets half the mean over list 1, one with only incoming edges
        # half the mean over list 0
        only_out, only_in = (deg0 == 0) & (deg1 > 0), (deg0 > 0) & (deg1 == 0)
        assert only_out.any() and only_in.any()
        for sel, col in ((only_out, 1), (only_in, 0)):
            for node in np.nonzero(sel)[0]:
                want = 0.5 * r64["ei"][case["flat"][:, col] == node].mean(axis=0)
                np.testing.assert_allclose(got["p"][node], want, rtol=1e-5)


@pytest.mark.parametrize("with_g_ni,with_g_ei", [(True, True), (False, True), (True, False)],
                         ids=["all", "no-g_ni", "no-g_ei"])
@pytest.mark.parametrize("name", sorted(mref.kernel_cases()))
def test_reverse_kernels_alone(name, with_g_ni, with_g_ei):
    case, f32, _ = _kernel_case(name)
    r32, r64 = _kernel_reverse(name, with_g_ni, with_g_ei)
    plan, splits = _plan(case)
    n, m, k, w = plan.N, plan.M, case["k"], case["w"]
    g = len(case["row_splits"]) - 1
    (ptr0, _, _), (ptr1, _, _) = plan.csr(0), plan.csr(1)
    x, z, p, ei = _cuda(case["x"]), _cuda(case["z"]), _cuda(f32["p"]), _cuda(f32["ei"])
    g_out = _cuda(case["g_out"])
    g_ni = _cuda(case["g_ni"]) if with_g_ni else None
    g_ei = _cuda(case["g_ei"]) if with_g_ei else None
    op = _ffi.MP_MEAN if case["pooling"] == "mean" else _ffi.MP_SUM

    def once():
        x_bar, z_bar, q, s_bar = _nan(n, w), _nan(n, k), _nan(n, k), _nan(m, k)
        _ffi.call("mp_megan_readout_grad_f32", _ffi.ptr(g_out), _ffi.ptr(g_ni), _ffi.ptr(x), _ffi.ptr(z), _ffi.ptr(p), n, k,
                  w, _ffi.ptr(splits), g, op, _ffi.ptr(x_bar), _ffi.ptr(z_bar), _ffi.ptr(q), _ffi.stream())
        _ffi.call("mp_megan_edge_importance_grad_f32", _ffi.ptr(g_ei), _ffi.ptr(q), _ffi.ptr(ei), _ffi.ptr(plan.cols),
                  _ffi.ptr(ptr0), _ffi.ptr(ptr1), n, m, k, _ffi.ptr(s_bar), _ffi.stream())
        return x_bar, z_bar, s_bar

    first, again = once(), once()
    torch.cuda.synchronize()
    for a, b in zip(first, again):
        assert torch.equal(a, b), "two runs differ"
    for what, t in zip(("x_bar", "z_bar", "s_bar"), first):
        got = t.cpu().numpy()
        assert got.shape == r64[what].shape and np.all(np.isfinite(got)), what
        assert_rows_close(_rows(got), _rows(r32[what]), _rows(r64[what]), what="%s %s" % (name, what))


def test_argument_checks_refuse_what_is_not_served():
    z9, x6 = torch.zeros((4, 9), device="cuda"), torch.zeros((4, 6), device="cuda")
    z2, x8 = torch.zeros((4, 2), device="cuda"), torch.zeros((4, 8), device="cuda")
    ptr = torch.zeros(5, dtype=torch.int32, device="cuda")
    splits = torch.tensor([0, 4], dtype=torch.int64, device="cuda")
    ni, out = torch.zeros((4, 9), device="cuda"), torch.zeros((1, 9 * 8), device="cuda")
    readout = lambda k, z, x, w: _ffi.call("mp_megan_readout_f32", None, 0, k, _ffi.ptr(ptr), None, _ffi.ptr(ptr), None,
                                           _ffi.ptr(z), _ffi.ptr(x), 4, w, _ffi.ptr(splits), 1, _ffi.MP_SUM, None,
                                           _ffi.ptr(ni), _ffi.ptr(out), _ffi.stream())
    with pytest.raises(ValueError, match="channels"):
        readout(9, z9, x8, 8)
    with pytest.raises(ValueError, match="multiple of 4"):
        readout(2, z2, x6, 6)
    with pytest.raises(ValueError, match="null pointer"):
        _ffi.call("mp_megan_readout_f32", None, 0, 2, None, None, None, None, None, None, 4, 8, _ffi.ptr(splits), 1,
                  _ffi.MP_SUM, None, None, _ffi.ptr(out), _ffi.stream())
    with pytest.raises(ValueError, match="null pointer"):
        _ffi.call("mp_megan_edge_importance_f32", 1, None, 3, 2, None, _ffi.stream())
    with pytest.raises(ValueError, match="null pointer"):
        _ffi.call("mp_megan_edge_importance_grad_f32", None, None, None, None, None, None, 4, 3, 2, None, _ffi.stream())
    with pytest.raises(ValueError, match="null pointer"):
        _ffi.call("mp_megan_readout_grad_f32", None, None, None, None, None, 4, 2, 8, None, 1, _ffi.MP_SUM, None, None,
                  None, _ffi.stream())
    readout(2, z2, x8, 8)                                    # served: no edges, four nodes
    torch.cuda.synchronize()
    assert torch.all(out[:, :16] == 0.0)
    # empty sizes
    _ffi.call("mp_megan_edge_importance_f32", 1, None, 0, 2, None, _ffi.stream())
    _ffi.call("mp_megan_readout_f32", None, 0, 2, None, None, None, None, None, None, 0, 8, None, 0, _ffi.MP_SUM, None, None,
              None, _ffi.stream())
    _ffi.call("mp_megan_readout_grad_f32", None, None, None, None, None, 0, 2, 8, None, 0, _ffi.MP_SUM, None, None, None,
              _ffi.stream())
    _ffi.call("mp_megan_edge_importance_grad_f32", None, None, None, None, None, None, 0, 0, 2, None, _ffi.stream())


# ------------------------------------------------------------------------------------------------ the model
def _build(cfg, seed=21, **extra):
    """(model, inputs, batch, parameter dictionary) of a configuration on 6 QM9-like graphs."""
    from gcnn_keras_amd.literature import MEGAN
    b, p = mref.model_case(cfg, seed=seed)
    inputs = list(INPUTS)
    if cfg["embed"] is not None:
        inputs[0] = dict(INPUTS[0], shape=(None,))
    model = MEGAN.make_model(inputs=inputs, **dict(mref.model_kwargs(cfg), **extra))
    model.set_weights(list(p.values()))
    x = [_rag(b["x"], b["node_splits"]), _rag(b["e"], b["edge_splits"]), _rag(b["edge_indices"], b["edge_splits"])]
    return model, x, b, p


@functools.lru_cache(maxsize=None)
def _model_refs(name, seed=21):
    cfg = dict(mref.model_cases(), **mref.unserved_cases())[name]
    b, p = mref.model_case(cfg, seed=seed)
    return [[t.numpy() for t in mref.model_restate(p, cfg, b, dt)] for dt in (torch.float32, torch.float64)]


def _assert_outputs(got, refs, what):
    out, ni, ei = got
    r32, r64 = refs
    for label, t, a32, a64 in zip(("out", "node importances", "edge importances"), (out, ni.values, ei.values), r32, r64):
        a = t.detach().cpu().numpy()
        assert a.shape == a64.shape, (what, label, a.shape, a64.shape)
        assert_rows_close(_rows(a), _rows(a32), _rows(a64), what="%s, %s" % (what, label))


@pytest.mark.parametrize("fused_attention", [True, False], ids=["attention-fused", "attention-layers"])
@pytest.mark.parametrize("fused_readout", [True, False], ids=["readout-fused", "readout-layers"])
@pytest.mark.parametrize("name", sorted(mref.model_cases()))
def test_model_on_both_routes(name, fused_readout, fused_attention):
    cfg = mref.model_cases()[name]
    model, x, b, p = _build(cfg)
    model.auto_graph = False
    model.use_fused_readout = fused_readout
    model.use_fused_attention = fused_attention
    served = name != "u5-3-k2"             # 6 columns: not a multiple of 4
    assert model.fused_readout is served
    with torch.no_grad():
        got = model(x)
    assert model.last_readout_route == ("fused" if fused_readout and served else "layers")
    g = len(b["node_splits"]) - 1
    assert tuple(got[0].shape) == (g, cfg["final_units"][-1])
    assert tuple(got[1].values.shape) == (int(b["node_splits"][-1]), cfg["k"])
    assert tuple(got[2].values.shape) == (int(b["edge_splits"][-1]), cfg["k"])
    _assert_outputs(got, _model_refs(name), "%s readout %s attention %s" % (name, fused_readout, fused_attention))


@pytest.mark.parametrize("name", sorted(mref.unserved_cases()))
def test_unserved_configurations_take_the_layer_sequence(name):
    cfg = mref.unserved_cases()[name]
    model, x, b, p = _build(cfg)
    assert model.use_fused_readout is True and model.fused_readout is False
    model.auto_graph = False
    with torch.no_grad():
        got = model(x)
    assert model.last_readout_route == "layers"
    _assert_outputs(got, _model_refs(name), name)


def test_eager_replay_predict_and_explain():
    name = "u32x3-k2-concat"
    model, x, b, p = _build(mref.model_cases()[name])
    with torch.no_grad():
        first = model(x)
        assert model.last_route == "eager" and model.last_readout_route == "fused"
        second = model(x)
        assert model.last_route == "graph"
        third = model(x)
        assert model.last_route == "graph"
        for a, c, d in zip(first, second, third):
            av, cv, dv = (t if torch.is_tensor(t) else t.values for t in (a, c, d))
            assert torch.equal(av, cv) and torch.equal(cv, dv)
            assert cv.data_ptr() != dv.data_ptr()             # fresh copies on replay, the ragged outputs included
        keep = second[1].values.clone()
        third[1].values.zero_()
        fourth = model(x)
        assert torch.equal(second[1].values, keep) and torch.equal(fourth[1].values, keep)
        ni, ei = model.explain_importances(x)
        assert torch.equal(ni.values, first[1].values) and torch.equal(ei.values, first[2].values)
        whole = model.predict(x)
        batched = model.predict(x, batch_size=4)
        for a, c in zip(whole, batched):
            av, cv = (t if torch.is_tensor(t) else t.values for t in (a, c))
            assert tuple(av.shape) == tuple(cv.shape)
            assert_rows_close(_rows(cv.cpu().numpy()), _rows(av.cpu().numpy()), what="predict in batches")
        assert np.array_equal(batched[1].row_splits_host(), b["node_splits"])
        # the output alone, eager and replayed
        model.return_importances = False
        alone = model(x)
        assert torch.is_tensor(alone) and torch.equal(alone, first[0])
        both = model(x, return_importances=True)
        assert len(both) == 3 and torch.equal(both[0], first[0])
    _assert_outputs(second, _model_refs(name), "replayed")


def test_weight_change_after_capture_and_the_switches():
    name = "u32x3-k2-concat"
    model, x, b, p = _build(mref.model_cases()[name], seed=31)
    with torch.no_grad():
        first = model(x)
        model(x)
        assert model.last_route == "graph"
    # weights changed in place: the replayed graph reads them where they are
    model.set_weights([0.5 * w for w in model.get_weights()])
    with torch.no_grad():
        replayed = model(x)
        assert model.last_route == "graph"
        model.auto_graph = False
        eager = model(x)
        model.auto_graph = True
    for a, c, d in zip(replayed, eager, first):
        av, cv, dv = (t if torch.is_tensor(t) else t.values for t in (a, c, d))
        assert torch.equal(av, cv) and not torch.equal(av, dv)
    # a flip of the readout switch drops the captured graphs: the next call is not a replay of the fused tail
    model.use_fused_readout = False
    with torch.no_grad():
        seq = model(x)
    assert model.last_route == "eager" and model.last_readout_route == "layers"
    model.use_fused_readout = True
    with torch.no_grad():
        model(x)
        assert model.last_route == "eager" and model.last_readout_route == "fused"
        model(x)
        assert model.last_route == "graph"
    # ... and so does the attention switch; a switch flipped behind the model's back keys the graphs
    model.use_fused_attention = False
    with torch.no_grad():
        att = model(x)
    assert model.last_route == "eager"
    model.use_fused_attention = True
    model.attention_layers[1].use_fused_attention = False
    with torch.no_grad():
        mixed = model(x)
    assert model.last_route == "eager" and model.use_fused_attention is False
    model.attention_layers[1].use_fused_attention = True
    model._use_fused_readout = False
    with torch.no_grad():
        behind = model(x)
    assert model.last_route == "eager" and model.last_readout_route == "layers"
    model._use_fused_readout = True
    for what, got in (("readout on the layers", seq), ("attention on the layers", att), ("one layer switched", mixed),
                      ("readout switched behind the model", behind)):
        for a, c in zip(got, eager):
            av, cv = (t if torch.is_tensor(t) else t.values for t in (a, c))
            assert_rows_close(_rows(av.cpu().numpy()), _rows(cv.cpu().numpy()), what=what)


def _attention_part(model, x):
    node, edge, edi = x
    h, alphas = node, []
    for lay in model.attention_layers:
        h, alpha = lay([h, edge, edi])
        alphas.append(alpha)
    return node, h, alphas, edi


@pytest.mark.parametrize("importance_units", [[], [16, 8]])
def test_launch_counts_of_the_fused_tail(importance_units):
    cfg = mref.config([32, 32, 32], k=2, importance_units=importance_units)
    model, x, b, p = _build(cfg)
    chain = len(importance_units) + 1
    with torch.no_grad():
        node, h, alphas, edi = _attention_part(model, x)
        model._tail_fused(h, alphas, edi)                          # plans and CSRs are built once per batch
        count = _ffi.launch_count()
        model._tail_fused(h, alphas, edi)
        fused = _ffi.launch_count() - count
        model._tail_layers(node, h, alphas, edi)
        count = _ffi.launch_count()
        model._tail_layers(node, h, alphas, edi)
        layers = _ffi.launch_count() - count
    print("[megan] tail launches: fused %d, layer sequence %d" % (fused, layers))
    assert fused == chain + 2
    assert layers >= chain + 3 * cfg["k"] + 5
    # on the tape: the reverses of the Dense chain plus exactly 2
    weights = [t for lay in model.node_importance_layers for _, t in lay.weights]
    for t in weights:
        t.requires_grad_(True)
    try:
        with torch.enable_grad():
            leaf = h.with_values(h.values.detach().clone().requires_grad_(True))
            logits = [a.with_values(a.values.detach().clone().requires_grad_(True)) for a in alphas]
            count = _ffi.launch_count()
            z = model._importance_chain(leaf, last_linear=True).values
            dense_forward = _ffi.launch_count() - count    # on a tape a Dense with an activation keeps its pre-activation
            count = _ffi.launch_count()
            torch.autograd.grad(z, [leaf.values] + weights, torch.ones_like(z))
            dense_reverse = _ffi.launch_count() - count
            count = _ffi.launch_count()
            out, ni, ei = model._tail_fused(leaf, logits, edi)
            assert _ffi.launch_count() - count == dense_forward + 2        # on the tape: the same two launches
            count = _ffi.launch_count()
            grads = torch.autograd.grad([out, ni.values, ei.values], [leaf.values] + weights + [a.values for a in logits],
                                        [torch.ones_like(out), torch.ones_like(ni.values), torch.ones_like(ei.values)])
            reverse = _ffi.launch_count() - count
    finally:
        for t in weights:
            t.requires_grad_(False)
    print("[megan] tail reverse launches: %d (Dense chain alone %d)" % (reverse, dense_reverse))
    assert reverse == dense_reverse + 2
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)


def test_second_order_request_raises():
    model, x, b, p = _build(mref.model_cases()["u32x3-k2-concat"])
    with torch.no_grad():
        node, h, alphas, edi = _attention_part(model, x)
    with torch.enable_grad():
        leaf = h.with_values(h.values.detach().clone().requires_grad_(True))
        out, ni, ei = model._tail_fused(leaf, alphas, edi)
        # (out * out): the upstream gradient 2 out is itself on the tape, so the rule's outputs are asked to be
        first, = torch.autograd.grad((out * out).sum(), leaf.values, create_graph=True)
        with pytest.raises(RuntimeError, match="once_differentiable"):
            first.sum().backward()


# ------------------------------------------------------------------------------------------------ training
TRAINING = {
    # regression with the explanation step: K = 2, limits and a reference, both extra loss terms
    "regression": (dict(units=[32, 32], k=2, importance_units=[8], regression_limits=(-1.0, 1.0), regression_reference=0.0,
                        importance_factor=1.0, importance_multiplier=2.0, sparsity_factor=0.1), "mean_squared_error"),
    # classification: one-hot target over K = 2 classes, probabilities from a sigmoid
    "classification": (dict(units=[32, 32], k=2, final_units=[2], final_activation="sigmoid", final_pooling="mean",
                            importance_factor=0.5, importance_multiplier=0.5, sparsity_factor=0.2), "binary_crossentropy"),
}


def _target(kind, rows=6):
    rng = np.random.default_rng(4)
    if kind == "regression":
        return rng.uniform(-1.0, 1.0, size=(rows, 1)).astype(np.float32)
    cls = rng.integers(0, 2, size=rows)
    return np.eye(2, dtype=np.float32)[cls]


def _ref_loss(w, p, cfg, b, y, loss, dt):
    params = dict(zip(p.keys(), w))
    x = torch.tensor(b["x"], dtype=dt)
    out, ni, _ = mref.model_forward(params, cfg, x, torch.tensor(b["e"], dtype=dt), b["flat"], b["node_splits"])
    return mref.total_loss(out, ni, torch.from_numpy(y).to(dt), b["node_splits"], cfg, loss)


@pytest.mark.parametrize("fused_readout", [True, False], ids=["readout-fused", "readout-layers"])
@pytest.mark.parametrize("kind", sorted(TRAINING))
def test_weight_gradients_match_restatement_autograd(kind, fused_readout):
    kw, loss_name = TRAINING[kind]
    cfg = mref.config(**kw)
    model, x, b, p = _build(cfg, seed=41, return_importances=False)
    model.use_fused_readout = fused_readout
    model.compile(optimizer="sgd", loss=loss_name)
    y = _target(kind)
    model.requires_grad_(True)
    try:
        with torch.enable_grad():
            loss, exp_loss = model.total_loss(x, _cuda(y))
            loss.backward()
        assert model.last_readout_route == ("fused" if fused_readout else "layers")
        grads = [None if t.grad is None else t.grad.detach().cpu().numpy() for t in model.trainable_weights]
    finally:
        model.requires_grad_(False)
        for t in model.trainable_weights:
            t.grad = None
    refs = {}
    for dt in (torch.float32, torch.float64):
        w = [torch.tensor(a, dtype=dt, requires_grad=True) for a in p.values()]
        total, exp = _ref_loss(w, p, cfg, b, y, loss_name, dt)
        refs[dt] = (float(total.detach()), float(exp.detach()), [g.numpy() for g in torch.autograd.grad(total, w)])
    np.testing.assert_allclose(float(loss.detach()), refs[torch.float64][0], rtol=1e-5)
    np.testing.assert_allclose(float(exp_loss.detach()), refs[torch.float64][1], rtol=1e-5)
    assert refs[torch.float64][1] != 0.0
    names = [n for n, _ in model.weights]
    assert len(names) == len(p)
    for name, g, g32, g64 in zip(names, grads, refs[torch.float32][2], refs[torch.float64][2]):
        assert g is not None, name
        assert_rows_close(_grad_rows(g), _grad_rows(g32), _grad_rows(g64), what="%s %s" % (kind, name))
        if np.max(np.abs(g64)) > 0:
            assert np.max(np.abs(g)) > 0, name


@pytest.mark.parametrize("fused_readout", [True, False], ids=["readout-fused", "readout-layers"])
def test_sgd_trajectory_tracks_the_restatement(fused_readout):
    kw, loss_name = TRAINING["regression"]
    cfg = mref.config(**kw)
    model, x, b, p = _build(cfg, seed=43, return_importances=False)
    model.use_fused_readout = fused_readout
    y = _target("regression")
    lr = 0.05
    model.compile(optimizer=torch.optim.SGD(model.trainable_weights, lr=lr), loss=loss_name)
    steps = [model.train_on_batch(x, y) for _ in range(5)]
    assert not any(t.requires_grad for t in model.trainable_weights)
    losses, exp_losses = [s[0] for s in steps], [s[1] for s in steps]
    assert model.last_exp_loss == exp_losses[-1]
    trajectories = {}
    for dt in (torch.float32, torch.float64):
        w = [torch.tensor(a, dtype=dt, requires_grad=True) for a in p.values()]
        opt = torch.optim.SGD(w, lr=lr)
        ref = []
        for _ in range(5):
            opt.zero_grad()
            total, exp = _ref_loss(w, p, cfg, b, y, loss_name, dt)
            total.backward()
            opt.step()
            ref.append((float(total.detach()), float(exp.detach())))
        trajectories[dt] = np.array(ref)
    r64, r32 = trajectories[torch.float64], trajectories[torch.float32]
    own = float(np.max(np.abs(r32 - r64) / np.abs(r64)))
    rtol = 1e-5 if own <= 1e-5 else 2 * own
    print("[megan] engine %s restatement %s (float32 restatement %.2e from float64, rtol %.1e)" % (
        losses, list(r64[:, 0]), own, rtol))
    np.testing.assert_allclose(losses, r64[:, 0], rtol=rtol)
    np.testing.assert_allclose(exp_losses, r64[:, 1], rtol=rtol)
    assert len(set(losses)) == 5
    # the trained weights on the inference routes
    with torch.no_grad():
        model.return_importances = True
        out, ni, ei = model(x)
        assert model.last_readout_route == ("fused" if fused_readout else "layers")
    assert bool(torch.isfinite(out).all())


def test_fit_records_the_explanation_loss():
    # the reference's co-training test: units [5, 3], two channels, regression limits (-1, 1) around 0
    cfg = mref.config([5, 3], k=2, regression_limits=(-1.0, 1.0), regression_reference=0.0, importance_factor=1.0)
    model, x, b, p = _build(cfg, seed=47, return_importances=False)
    model.compile(optimizer="adam", loss="mean_squared_error")
    y = _target("regression")
    history = model.fit(x, y, batch_size=2, epochs=2, seed=1)
    assert set(history.history) == {"loss", "exp_loss"}
    assert len(history.history["loss"]) == 2 and len(history.history["exp_loss"]) == 2
    assert all(np.isfinite(v) for v in history.history["loss"] + history.history["exp_loss"])
    assert all(v != 0.0 for v in history.history["exp_loss"])
    assert model.last_exp_loss is not None and model.last_exp_loss != 0.0
    plain = _build(mref.config([5, 3], k=2), seed=47, return_importances=False)[0]
    plain.compile(optimizer="adam", loss="mean_squared_error")
    assert set(plain.fit(x, y, batch_size=3, epochs=1, seed=1).history) == {"loss"} and plain.last_exp_loss is None
    with pytest.raises(NotImplementedError, match="return_importances=True"):
        supervised = _build(cfg, seed=47)[0]
        supervised.compile(optimizer="adam", loss="mean_squared_error")
        supervised.train_on_batch(x, y)
    with pytest.raises(NotImplementedError, match="dropout"):
        dropped = _build(cfg, seed=47, return_importances=False, dropout_rate=0.1)[0]
        dropped.compile(optimizer="adam", loss="mean_squared_error")
        dropped.train_on_batch(x, y)
    with torch.no_grad():           # inference with dropout configured: the identity
        quiet = _build(cfg, seed=47, dropout_rate=0.1, final_dropout_rate=0.1)[0]
        assert len(quiet(x)) == 3
