"""RGCN / GNNFilm on csrc/mp_rgcn.hip: the fused relational step through the C ABI in both modes,
``DecomposedRelationalDense`` (``num_bases`` / ``num_blocks``; forward and gradients), the layers and the models on both
routes, graph replay and training through the layer sequence, all against tests/rgcn_reference.py (float32 and float64).
Index lists come from tests/topologies.py.

Bars: rows through ``parity.assert_rows_close``; FiLM receivers without edges exactly ``act(0)``; weight updates under the
bar of tests/test_gpu_gat.py's one-step test."""
import functools

import numpy as np
import pytest
import torch

import rgcn_reference as ref
import topologies as topo
from gcnn_keras_amd import _ffi
from parity import assert_rows_close

pytestmark = pytest.mark.gpu

MODES = {"rgcn": _ffi.MP_RELCONV_RGCN, "film": _ffi.MP_RELCONV_FILM}


def _rag(values, splits):
    from gcnn_keras_amd.ragged import RaggedTensor
    return RaggedTensor.from_numpy(values, splits)


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ the kernel alone
@functools.lru_cache(maxsize=None)
def _kernel_case(name):
    return ref.kernel_case(**ref.kernel_cases()[name])


@functools.lru_cache(maxsize=None)
def _kernel_refs(name, mode):
    case = _kernel_case(name)
    return ref.kernel_restate(case, mode, torch.float32), ref.kernel_restate(case, mode, torch.float64)


def _run_kernel(case, mode):
    """The entry point twice on NaN-filled outputs; ``(out, perm0)``."""
    nodes = _rag(case["nodes"], case["row_splits"])
    idx = _rag(case["indices"], case["index_splits"])
    plan = idx.index_plan(nodes)
    plan.validate()
    ptr0, perm0, _ = plan.csr(0)
    n, e, k, u = plan.N, plan.M, case["k"], case["u"]
    assert n == case["rows"] and e == len(case["flat"])
    p = {key: _cuda(v) for key, v in case["params"].items()}
    rel = _cuda(case["rel"])
    w = _cuda(case["edge_weights"]) if mode == "rgcn" else None
    code = lambda name: _ffi.activation_code(name)

    def once():
        out = torch.full((n, u), float("nan"), device="cuda")          # every row has to be written
        _ffi.call("mp_relational_conv_f32", MODES[mode], _ffi.ptr(nodes.values), n, k, _ffi.ptr(plan.cols), e,
                  _ffi.ptr(ptr0), _ffi.ptr(perm0), _ffi.ptr(rel), _ffi.ptr(w), case["r"], _ffi.ptr(p["kernel"]),
                  _ffi.ptr(p["bias"]), u, _ffi.ptr(p["w0"]), _ffi.ptr(p["b0"]), code(case["act0"]), _ffi.ptr(p["wg"]),
                  _ffi.ptr(p["bg"]), _ffi.ptr(p["wt"]), _ffi.ptr(p["bt"]), code(case["act_m"]), code(case["act"]), 0.05,
                  _ffi.ptr(out), _ffi.stream())
        return out

    first, again = once(), once()
    torch.cuda.synchronize()
    assert torch.equal(first, again), "two runs differ"
    return first.cpu().numpy(), perm0


@pytest.mark.parametrize("mode", ["rgcn", "film"])
@pytest.mark.parametrize("name", sorted(ref.kernel_cases()))
def test_kernel_against_the_restatement(name, mode):
    case = _kernel_case(name)
    r32, r64 = _kernel_refs(name, mode)
    out, perm0 = _run_kernel(case, mode)
    if "shuffled" in name:
        assert perm0 is not None
    assert out.shape == r64.shape and np.all(np.isfinite(out))
    err = assert_rows_close(out, r32, r64, what="%s %s" % (mode, name))
    print("[rgcn] %s %s: worst row %.2e from the float32 restatement" % (mode, name, err))
    lonely = topo.in_degrees(case["flat"], case["rows"]) == 0
    if lonely.any():
        want = ref.no_edge_rows(case, mode)[lonely]
        if mode == "film":
            assert np.array_equal(out[lonely], want.astype(np.float32))          # act(0), exactly
        else:
            assert_rows_close(out[lonely], want.astype(np.float32), want, what="%s %s, rows without edges" % (mode, name))


# ------------------------------------------------------------------- RelationalDense with num_bases / num_blocks
@pytest.mark.parametrize("bases,blocks", [(3, None), (None, 2), (3, 2)], ids=["bases", "blocks", "both"])
def test_relational_dense_decompositions_forward_and_gradients(bases, blocks):
    from gcnn_keras_amd.layers.relational import DecomposedRelationalDense
    rng = np.random.default_rng(17)
    rows, k, u, r = 75, 12, 8, 5
    splits = np.array([0, 40, 40, 75], np.int64)
    x = rng.normal(size=(rows, k)).astype(np.float32)
    rel = rng.integers(0, r, size=rows).astype(np.int64)
    rel[3], rel[50] = -1, r
    g = rng.normal(size=(rows, u)).astype(np.float32)
    lay = DecomposedRelationalDense(u, num_relations=r, num_bases=bases, num_blocks=blocks, activation="tanh")
    lay.ensure_built([(None, None, k), (None, None)])
    names = [n for n, _ in lay.weights]
    assert names == ["kernel"] + (["lin_bases"] if bases else []) + ["bias"]
    values = [rng.normal(size=tuple(t.shape)).astype(np.float32) * 0.4 for _, t in lay.weights]
    lay.set_weights(values)

    xr, rr = _rag(x, splits), _rag(rel, splits)
    with torch.no_grad():
        plain = lay([xr, rr]).values.cpu().numpy()
    tensors = [t for _, t in lay.weights]
    for t in tensors:
        t.requires_grad_(True)
    xr.values.requires_grad_(True)
    try:
        with torch.enable_grad():
            y = lay([xr, rr]).values
            grads = torch.autograd.grad((y * _cuda(g)).sum(), tensors + [xr.values])
        grads = [t.cpu().numpy() for t in grads]
        taped = y.detach().cpu().numpy()
    finally:
        for t in tensors:
            t.requires_grad_(False)
    refs = []
    for dt in (torch.float32, torch.float64):
        w = dict(zip(names, [torch.tensor(v, dtype=dt, requires_grad=True) for v in values]))
        xx = torch.tensor(x, dtype=dt, requires_grad=True)
        yy = ref.relational_dense(xx, rel, w["kernel"], w["bias"], "tanh", w.get("lin_bases"), blocks)
        order = [w[n] for n in names] + [xx]
        gr = torch.autograd.grad((yy * torch.tensor(g, dtype=dt)).sum(), order)
        refs.append((yy.detach().numpy(), [t.numpy() for t in gr]))
    assert np.array_equal(plain, taped)
    assert_rows_close(plain, refs[0][0], refs[1][0], what="RelationalDense y")
    for name, got, g32, g64 in zip(names + ["x"], grads, refs[0][1], refs[1][1]):
        assert got.shape == g64.shape, name
        rows2d = (lambda a: a.reshape(-1, a.shape[-1])) if got.ndim > 1 else (lambda a: a[None])
        assert_rows_close(rows2d(got), rows2d(g32), rows2d(g64), what="RelationalDense d%s" % name)
        assert np.max(np.abs(got)) > 0, name


# ------------------------------------------------------------------------------------------------ layers
def _both_routes(layer, inputs):
    with torch.no_grad():
        layer.use_fused_relational = True
        layer(inputs)                         # plans and CSRs are built once per batch
        count = _ffi.launch_count()
        fused = layer(inputs)
        fused_launches = _ffi.launch_count() - count
        layer.use_fused_relational = False
        count = _ffi.launch_count()
        seq = layer(inputs)
        seq_launches = _ffi.launch_count() - count
        layer.use_fused_relational = True
    return fused.values.cpu().numpy(), fused_launches, seq.values.cpu().numpy(), seq_launches


@pytest.mark.parametrize("mode", ["rgcn", "film"])
@pytest.mark.parametrize("name", ["n33-shuffled-r64-empty-graphs", "chunks-sorted-r20-oor", "n17-shuffled-r3-oor"])
def test_layer_on_both_routes(name, mode):
    from gcnn_keras_amd.layers.conv.rgcn_conv import GNNFilmStep, RGCNStep
    case = _kernel_case(name)
    p, k, u, r = case["params"], case["k"], case["u"], case["r"]
    nodes, idx = _rag(case["nodes"], case["row_splits"]), _rag(case["indices"], case["index_splits"])
    rel = _rag(case["rel"], case["index_splits"])
    if mode == "rgcn":
        layer = RGCNStep(dense_kwargs={"units": u, "activation": case["act0"]},
                         dense_relation_kwargs={"units": u, "num_relations": r},
                         activation_kwargs={"activation": case["act"]})
        inputs = [nodes, idx, _rag(case["edge_weights"], case["index_splits"]), rel]
        shapes = [(None, None, k), (None, None, 2), (None, None, 1), (None, None)]
        weights = [p["w0"], p["b0"], p["kernel"], p["bias"]]
    else:
        layer = GNNFilmStep(dense_relation_kwargs={"units": u, "num_relations": r},
                            dense_modulation_kwargs={"units": u, "num_relations": r, "activation": case["act_m"]},
                            activation_kwargs={"activation": case["act"]})
        inputs = [nodes, idx, rel]
        shapes = [(None, None, k), (None, None, 2), (None, None)]
        weights = [p["wg"], p["bg"], p["wt"], p["bt"], p["kernel"], p["bias"]]
    layer.ensure_built(shapes)
    assert layer.fused_relational is True
    layer.set_weights(weights)
    fused, fused_launches, seq, seq_launches = _both_routes(layer, inputs)
    print("[rgcn] %s layer: launches fused %d, layer sequence %d" % (mode, fused_launches, seq_launches))
    assert fused_launches == 1 and seq_launches > 4
    r32, r64 = _kernel_refs(name, mode)
    assert_rows_close(fused, r32, r64, what="%s layer, fused" % mode)
    assert_rows_close(seq, r32, r64, what="%s layer, layer sequence" % mode)


# ------------------------------------------------------------------------------------------------ models
def _make(kind):
    from gcnn_keras_amd.literature import GNNFilm, RGCN
    return RGCN.make_model if kind == "rgcn" else GNNFilm.make_model


def _model_inputs(kind, b):
    x = [_rag(b["x"], b["node_splits"]), _rag(b["edge_indices"], b["edge_splits"])]
    if kind == "rgcn":
        x.append(_rag(b["edge_weights"], b["edge_splits"]))
    return x + [_rag(b["edge_relations"], b["edge_splits"])]


def _model_case(kind, name):
    kw, fwd, seed = ref.model_cases(kind)[name]
    model = _make(kind)(**kw)
    ws, b = ref.parity_weights(model, seed), ref.model_batch(fwd["embed"], seed)
    model.set_weights(ws)
    return model, _model_inputs(kind, b), b, ws, fwd


def _values(out):
    return (out if torch.is_tensor(out) else out.values).detach().cpu().numpy()


@pytest.mark.parametrize("kind", ["rgcn", "film"])
@pytest.mark.parametrize("name", ["default-graph", "wide-node", "bases-blocks"])
def test_model_on_both_routes(kind, name):
    model, x, b, ws, fwd = _model_case(kind, name)
    assert model.fused_relational_blocks == [True, True]
    model.auto_graph = False
    with torch.no_grad():
        model(x)
        count = _ffi.launch_count()
        fused = _values(model(x))
        fused_launches = _ffi.launch_count() - count
        model.use_fused_relational = False
        count = _ffi.launch_count()
        seq = _values(model(x))
        seq_launches = _ffi.launch_count() - count
        model.use_fused_relational = True
    print("[rgcn] %s %s: launches per forward: fused %d, layer sequence %d" % (kind, name, fused_launches, seq_launches))
    assert fused_launches < seq_launches
    r32, r64 = (ref.model_forward(kind, ws, b, dt, **fwd).numpy() for dt in (torch.float32, torch.float64))
    assert fused.shape == r64.shape == ((4, 2) if fwd.get("output_embedding", "graph") == "graph" else (92, 2))
    assert_rows_close(fused, r32, r64, what="%s %s, fused" % (kind, name))
    assert_rows_close(seq, r32, r64, what="%s %s, layer sequence" % (kind, name))


@pytest.mark.parametrize("kind", ["rgcn", "film"])
def test_graph_replay_the_switches_and_a_call_under_grad(kind):
    model, x, b, ws, fwd = _model_case(kind, "bases-blocks")
    with torch.no_grad():
        first = model(x)
        assert model.last_route == "eager"
        second = model(x)
        assert model.last_route == "graph"
        third = model(x)
        assert model.last_route == "graph"
        assert torch.equal(first, second) and torch.equal(second, third)
    # weights changed in place: the replayed graph assembles the effective kernels from them again
    model.set_weights([0.5 * w for w in model.get_weights()])
    with torch.no_grad():
        replayed = model(x)
        assert model.last_route == "graph"
        model.auto_graph = False
        eager = model(x)
        model.auto_graph = True
    assert torch.equal(replayed, eager) and not torch.equal(replayed, first)
    # the model switch drops the captured graphs: the next call runs the layer sequence, not a replay of the fused route
    model.use_fused_relational = False
    with torch.no_grad():
        seq = model(x)
    assert model.last_route == "eager"
    model.use_fused_relational = True
    assert_rows_close(seq.cpu().numpy(), eager.cpu().numpy(), what="layer sequence after the switch")
    # a per-block switch is part of a captured graph's identity too
    model.relational_layers[1].use_fused_relational = False
    with torch.no_grad():
        mixed = model(x)
    assert model.last_route == "eager" and model.use_fused_relational is False
    model.relational_layers[1].use_fused_relational = True
    assert_rows_close(mixed.cpu().numpy(), eager.cpu().numpy(), what="one block on the layer sequence")
    # a call under grad takes the layer sequence: the output is on the tape and the launches are those of that route
    model.auto_graph = False
    with torch.no_grad():
        count = _ffi.launch_count()
        model(x)
        fused_launches = _ffi.launch_count() - count
    model.requires_grad_(True)
    try:
        with torch.enable_grad():
            count = _ffi.launch_count()
            taped = model(x)
            taped_launches = _ffi.launch_count() - count
        assert taped.grad_fn is not None and taped_launches > fused_launches
    finally:
        model.requires_grad_(False)
    assert_rows_close(taped.detach().cpu().numpy(), eager.cpu().numpy(), what="call under grad")


# ------------------------------------------------------------------------------------------------ training
def _mse(pred, target):
    return torch.square(pred - target).mean(dim=-1).mean()


@pytest.mark.parametrize("kind", ["rgcn", "film"])
@pytest.mark.parametrize("bases", [None, 3], ids=["plain", "bases"])
def test_one_training_step(kind, bases):
    """One SGD step under mean squared error on feature inputs (K = 32, U = 64, depth 2) against the float64
    restatement's step."""
    spec = [dict(s) for s in (ref.RGCN_INPUTS if kind == "rgcn" else ref.FILM_INPUTS)]
    spec[0]["shape"] = (None, 32)
    rel = {"units": 64, "num_relations": 20}
    if bases:
        rel["num_bases"] = bases
    model = _make(kind)(inputs=spec, depth=2, dense_relation_kwargs=rel, output_mlp=ref.OUTPUT_MLP)
    ws, b = ref.parity_weights(model, 51), ref.model_batch(False, 51)
    model.set_weights(ws)
    x = _model_inputs(kind, b)
    target = np.random.default_rng(6).uniform(-1.0, 1.0, size=(4, 2)).astype(np.float32)
    lr = 0.05
    model.compile(optimizer=torch.optim.SGD(model.trainable_weights, lr=lr), loss="mean_squared_error")
    loss = model.train_on_batch(x, target)
    after = model.get_weights()
    assert not any(t.requires_grad for t in model.trainable_weights)
    w = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in ws]
    out = ref.model_forward(kind, w, b, torch.float64, depth=2, embed=False, num_bases=bases)
    want_loss = _mse(out, torch.from_numpy(target).double())
    grads = torch.autograd.grad(want_loss, w)
    np.testing.assert_allclose(loss, float(want_loss.detach()), rtol=1e-5)
    for (name, _), got, t0, g in zip(model.weights, after, w, grads):
        want = (t0.detach() - lr * g).numpy()
        step = float(np.max(np.abs(lr * g.numpy())))
        assert step > 0, name
        # tests/test_gpu_gat.py::test_one_step_under_binary_crossentropy: 5e-5 of the tensor's largest step plus two float32
        # ulps of the stored weight
        assert np.max(np.abs(got - want)) <= 5e-5 * step + 2.4e-7 * float(np.max(np.abs(want))), name
    # the fused route serves the trained weights
    with torch.no_grad():
        fused = _values(model(x))
    r32, r64 = (ref.model_forward(kind, after, b, dt, depth=2, embed=False, num_bases=bases).numpy()
                for dt in (torch.float32, torch.float64))
    assert_rows_close(fused, r32, r64, what="%s trained weights, fused" % kind)
