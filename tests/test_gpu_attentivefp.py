"""AttentiveFP on the GPU: the edge-feature head's two kernels and the readout kernel through the C ABI, the GRU combine's
reverse kernel, the new reverse paths of ``GRUUpdate`` and ``PoolingNodesAttention``, both routes of the layers and the
model, graph replay, and training against the torch restatement (tests/attentivefp_reference.py) in float32 with its
float64 twin.  Rows are compared through ``parity.assert_rows_close`` with its default bars."""
import functools

import numpy as np
import pytest
import torch

import attentivefp_reference as aref
import topologies as topo
from gcnn_keras_amd import _ffi
from parity import assert_rows_close, max_rel

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64


def _rag(values, splits):
    from gcnn_keras_amd.ragged import RaggedTensor
    return RaggedTensor.from_numpy(values, splits)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _logits_close(got, r32, r64, what):
    if r64.size == 0:
        assert got.size == 0
        return
    err, e32 = max_rel(got, r64), max_rel(r32, r64)
    print("[attentivefp] %s: logits %.2e of the tensor from float64 (float32 restatement %.2e)" % (what, err, e32))
    assert err <= max(2e-6, 4 * e32), what


# ------------------------------------------------------------------------------------------------ edge head kernels
@functools.lru_cache(maxsize=None)
def _edge_case(name):
    case = aref.edge_case(**aref.edge_cases()[name])
    return case, aref.edge_restate(case, F32), aref.edge_restate(case, F64)


def _run_edge_kernels(case):
    """Node-side products by ``dense_values`` on row-block views, then the two entry points; ``(out, logits in edge
    order, perm0)``."""
    from gcnn_keras_amd.layers.modules import dense_values
    nodes = _rag(case["nodes"], case["row_splits"])
    idx = _rag(case["indices"], case["index_splits"])
    plan = idx.index_plan(nodes)
    plan.validate()
    ptr0, perm0, _ = plan.csr(0)
    n, e, u, d, f = plan.N, plan.M, case["u"], case["d"], case["nodes"].shape[1]
    hv, gv = nodes.values, _cuda(case["edges"])
    w = {k: _cuda(v) for k, v in case["params"].items()}
    w2, wa = w["fc2/kernel"], w["alpha_activation/kernel"]
    x = dense_values(hv, w2[:f], None)
    a1 = dense_values(hv, w["fc1/kernel"], w.get("fc1/bias"), case["act"])
    p = dense_values(a1, wa[:u], None)
    code, ctx = _ffi.activation_code(case["act"]), _ffi.activation_code(case["act_context"])

    def once():
        logit = torch.full((e,), float("nan"), device="cuda")           # every entry has to be written
        msg = torch.full((e, u), float("nan"), device="cuda")
        out = torch.full((n, u), float("nan"), device="cuda")
        _ffi.call("mp_afp_edge_f32", u, _ffi.ptr(x), _ffi.ptr(p), n, _ffi.ptr(gv), d, _ffi.ptr(w2[f:]),
                  _ffi.ptr(w.get("fc2/bias")), _ffi.ptr(w["linear_trafo/kernel"]), _ffi.ptr(w.get("linear_trafo/bias")),
                  _ffi.ptr(wa[u:]), _ffi.ptr(w.get("alpha_activation/bias")), _ffi.ptr(w["alpha/kernel"]),
                  _ffi.ptr(plan.cols), e, _ffi.ptr(perm0), code, 0.05, _ffi.ptr(logit), _ffi.ptr(msg), _ffi.stream())
        _ffi.call("mp_afp_attend_f32", u, _ffi.ptr(msg), _ffi.ptr(logit), n, _ffi.ptr(plan.cols), e, _ffi.ptr(ptr0),
                  _ffi.ptr(perm0), ctx, 0.05, _ffi.ptr(out), _ffi.stream())
        return out, logit, msg

    first, again = once(), once()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, again)), "two runs differ"
    by_position = first[1].cpu().numpy()
    logits = np.empty_like(by_position)
    logits[perm0.cpu().numpy() if perm0 is not None else np.arange(e)] = by_position
    assert np.all(np.isfinite(first[2].cpu().numpy()))
    return first[0].cpu().numpy(), logits, perm0


@pytest.mark.parametrize("name", sorted(aref.edge_cases()))
def test_edge_head_kernels_against_the_restatement(name):
    case, (o32, l32), (o64, l64) = _edge_case(name)
    out, logits, perm0 = _run_edge_kernels(case)
    if "shuffled" in name:
        assert perm0 is not None
    elif "sorted" in name:
        assert perm0 is None
    assert out.shape == o64.shape and logits.shape == l64.shape
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(logits))
    _logits_close(logits, l32, l64, name)
    assert_rows_close(out, o32, o64, what=name)
    lonely = topo.in_degrees(case["flat"], case["rows"]) == 0
    assert np.all(out[lonely] == 0.0) and (lonely.any() or name.startswith("exact"))   # act_context(0) = 0 for all three


# ------------------------------------------------------------------------------------------------ readout kernel
@functools.lru_cache(maxsize=None)
def _readout_case(name):
    case = aref.readout_case(**aref.readout_cases()[name])
    return case, aref.readout_restate(case, F32), aref.readout_restate(case, F64)


def _readout_call(vals, splits, rows, w, case, out, term):
    from gcnn_keras_amd.layers.modules import dense_values
    from gcnn_keras_amd.ops.segment import reduce_op_code
    n, u = int(vals.shape[0]), case["u"]
    wn = dense_values(vals, w["linear_trafo/kernel"], w.get("linear_trafo/bias")) if n > 0 else None
    bias = w.get("gru/bias")
    _ffi.call("mp_afp_readout_f32", _ffi.ptr(vals), _ffi.ptr(wn), n, _ffi.ptr(splits), rows, u, case["depth"],
              reduce_op_code(case["pooling_method"]), _ffi.ptr(w["alpha/kernel"]), _ffi.ptr(w.get("alpha/bias")),
              _ffi.ptr(w["gru/kernel"]), _ffi.ptr(w["gru/recurrent_kernel"]),
              _ffi.ptr(None if bias is None else bias[0]), _ffi.ptr(None if bias is None else bias[1]),
              _ffi.activation_code(case["act"]), 0.05, _ffi.activation_code(case["act_context"]),
              _ffi.activation_code("tanh"), _ffi.activation_code("sigmoid"), _ffi.ptr(term), _ffi.ptr(out), _ffi.stream())


def _run_readout(case):
    vals, splits = _cuda(case["nodes"]), _cuda(case["row_splits"])
    rows = aref.graph_rows(case["row_splits"])
    w = {k: _cuda(v) for k, v in case["params"].items()}

    def once():
        out = torch.full((rows, case["u"]), float("nan"), device="cuda")     # every row has to be written
        term = torch.full((max(len(case["nodes"]), 1),), float("nan"), dtype=torch.float64, device="cuda")
        _readout_call(vals, splits, rows, w, case, out, term)
        return out

    first, again = once(), once()
    torch.cuda.synchronize()
    assert torch.equal(first, again), "two runs differ"
    return first.cpu().numpy()


def _readout_layer(case):
    from gcnn_keras_amd.layers.conv.attentivefp_conv import PoolingNodesAttentive
    layer = PoolingNodesAttentive(case["u"], depth=case["depth"], pooling_method=case["pooling_method"],
                                  activation=case["act"], activation_context=case["act_context"],
                                  use_bias="alpha/bias" in case["params"])
    layer.ensure_built((None, None, case["u"]))
    layer.set_weights(list(case["params"].values()))
    return layer


@pytest.mark.parametrize("name", sorted(aref.readout_cases()))
def test_readout_kernel_against_the_restatement_and_the_layer_sequence(name):
    case, r32, r64 = _readout_case(name)
    out = _run_readout(case)
    assert out.shape == r64.shape and np.all(np.isfinite(out))
    assert_rows_close(out, r32, r64, what=name)
    layer, x = _readout_layer(case), _rag(case["nodes"], case["row_splits"])
    with torch.no_grad():
        count = _ffi.launch_count()
        fused = layer(x)
        fused_launches = _ffi.launch_count() - count
        layer.use_fused_attentive = False
        count = _ffi.launch_count()
        seq = layer(x)
        seq_launches = _ffi.launch_count() - count
    assert np.array_equal(fused.cpu().numpy(), out)                      # the layer's fused route is this call
    assert fused_launches <= 2 and fused_launches < seq_launches         # one Dense launch and the kernel
    assert_rows_close(out, seq.cpu().numpy(), r64, what=name + ", against %d iterations of the layer sequence" % case["depth"])


def test_readout_kernel_on_graphs_without_nodes():
    """``N = 0``: through the C ABI every graph gets the recurrence on ``cont = act_context(0)`` from the zero state; the
    layer drops the trailing empty graphs, i.e. all of them."""
    case = aref.readout_case([0, 0, 0], u=32, depth=2)
    w = {k: _cuda(v) for k, v in case["params"].items()}
    out = torch.full((3, 32), float("nan"), device="cuda")
    term = torch.zeros(1, dtype=torch.float64, device="cuda")
    _readout_call(_cuda(case["nodes"]), _cuda(case["row_splits"]), 3, w, case, out, term)
    refs = []
    for dt in (F32, F64):
        p, h = aref.params_to(case["params"], dt), torch.zeros((3, 32), dtype=dt)
        for _ in range(2):
            h = aref.gru_cell(torch.zeros((3, 32), dtype=dt), h, p)
        refs.append(h.numpy())
    assert_rows_close(out.cpu().numpy(), *refs, what="graphs without nodes")
    layer = _readout_layer(case)
    with torch.no_grad():
        for fused in (True, False):
            layer.use_fused_attentive = fused
            assert tuple(layer(_rag(case["nodes"], case["row_splits"])).shape) == (0, 32)


# ------------------------------------------------------------------------------------------------ GRU reverse
def _gru_combine_ref(mx, mh, h, act, rec):
    u = h.shape[1]
    fa, fr = aref.ACTIVATIONS[act], aref.ACTIVATIONS[rec]
    z, r = fr(mx[:, :u] + mh[:, :u]), fr(mx[:, u:2 * u] + mh[:, u:2 * u])
    return z * h + (1.0 - z) * fa(mx[:, 2 * u:] + r * mh[:, 2 * u:])


@pytest.mark.parametrize("acts", [("tanh", "sigmoid"), ("softplus", "tanh")], ids=["tanh-sigmoid", "softplus-tanh"])
@pytest.mark.parametrize("u", [4, 32, 36])
@pytest.mark.parametrize("rows", [0, 1, 63, 64, 65])
def test_gru_combine_reverse(rows, u, acts):
    from gcnn_keras_amd.autograd import GRUCombine
    rng = np.random.default_rng(100 * rows + u)
    mx, mh = (rng.normal(size=(rows, 3 * u)).astype(np.float32) for _ in range(2))
    h, g = (rng.normal(size=(rows, u)).astype(np.float32) for _ in range(2))
    act, rec = _ffi.activation_code(acts[0]), _ffi.activation_code(acts[1])
    plain = torch.full((rows, u), float("nan"), device="cuda")
    dev = [_cuda(a) for a in (mx, mh, h)]                       # held: a pointer alone keeps no tensor alive
    _ffi.call("mp_gru_combine_f32", _ffi.ptr(dev[0]), _ffi.ptr(dev[1]), _ffi.ptr(dev[2]), rows, u, act, rec,
              _ffi.ptr(plain), _ffi.stream())
    leaves = [_cuda(a).requires_grad_(True) for a in (mx, mh, h)]
    out = GRUCombine.apply(*leaves, act, rec)
    assert torch.equal(out.detach(), plain)                     # the tape does not change the forward's bits
    grads = torch.autograd.grad(out, leaves, _cuda(g))
    assert [tuple(t.shape) for t in grads] == [(rows, 3 * u), (rows, 3 * u), (rows, u)]
    h_only, = torch.autograd.grad(GRUCombine.apply(_cuda(mx), _cuda(mh), leaves[2], act, rec), leaves[2], _cuda(g))
    assert torch.equal(h_only, grads[2])
    if rows == 0:
        return
    refs = []
    for dt in (F32, F64):
        t = [torch.tensor(a, dtype=dt, requires_grad=True) for a in (mx, mh, h)]
        o = _gru_combine_ref(*t, *acts)
        refs.append([o.detach().numpy()] + [x.numpy() for x in torch.autograd.grad(o, t, torch.tensor(g, dtype=dt))])
    assert_rows_close(plain.cpu().numpy(), refs[0][0], refs[1][0], what="gru combine")
    for k, what in enumerate(("d_mx", "d_mh", "d_h")):
        assert_rows_close(grads[k].cpu().numpy(), refs[0][k + 1], refs[1][k + 1], what="gru combine reverse, " + what)


def _gradient_close(name, got, g32, g64):
    """A gradient tensor against float64 autograd, in units of the tensor's largest entry (the bar of the GAT tests)."""
    assert got is not None, name
    scale = max(float(np.max(np.abs(g64))), 1e-3)
    e32 = float(np.max(np.abs(g32 - g64))) / scale
    err = float(np.max(np.abs(got - g64))) / scale
    print("[attentivefp] %s: gradient %.2e of its scale from float64 (float32 restatement %.2e)" % (name, err, e32))
    assert err <= max(1e-5, min(4 * e32, 5e-5)), name
    if np.max(np.abs(g64)) > 0:
        assert np.max(np.abs(got)) > 0, name


def test_gru_update_weight_and_input_gradients():
    from gcnn_keras_amd.layers.conv.mpnn_conv import GRUUpdate
    rng = np.random.default_rng(31)
    splits = np.array([0, 70, 71, 71, 92], np.int64)
    hs, xs = rng.normal(size=(92, 32)).astype(np.float32), rng.normal(size=(92, 20)).astype(np.float32)
    g = rng.normal(size=(92, 32)).astype(np.float32)
    p = aref.gru_params(rng, 20, 32)
    layer = GRUUpdate(32)
    layer.ensure_built([(None, None, 32), (None, None, 20)])
    layer.set_weights(list(p.values()))
    with torch.no_grad():
        plain = layer([_rag(hs, splits), _rag(xs, splits)]).values
    h, x = _rag(hs, splits), _rag(xs, splits)
    leaves = [h.values.requires_grad_(True), x.values.requires_grad_(True)] + [t.requires_grad_(True) for _, t in layer.weights]
    try:
        out = layer([h, x]).values
        grads = torch.autograd.grad(out, leaves, _cuda(g))
    finally:
        for _, t in layer.weights:
            t.requires_grad_(False)
    assert torch.equal(out.detach(), plain)
    refs = []
    for dt in (F32, F64):
        t = [torch.tensor(a, dtype=dt, requires_grad=True) for a in (hs, xs)]
        w = {k: torch.tensor(v, dtype=dt, requires_grad=True) for k, v in p.items()}
        o = aref.gru_cell(t[1], t[0], w)
        refs.append([o.detach().numpy()] + [v.numpy() for v in torch.autograd.grad(o, t + list(w.values()), torch.tensor(g, dtype=dt))])
    assert_rows_close(plain.cpu().numpy(), refs[0][0], refs[1][0], what="GRUUpdate")
    names = ["state", "updates", "kernel", "recurrent_kernel", "bias"]
    for k, name in enumerate(names):
        _gradient_close("GRUUpdate " + name, grads[k].cpu().numpy(), refs[0][k + 1], refs[1][k + 1])


def test_pooling_nodes_attention_gradients():
    from gcnn_keras_amd.layers.pooling import PoolingNodesAttention
    rng = np.random.default_rng(33)
    splits = np.array([0, 0, 70, 71, 71, 92, 92], np.int64)          # empty first, interior and last
    nodes, logits = rng.normal(size=(92, 12)).astype(np.float32), rng.normal(size=(92, 1)).astype(np.float32)
    g = rng.normal(size=(5, 12)).astype(np.float32)
    layer = PoolingNodesAttention()
    with torch.no_grad():
        plain = layer([_rag(nodes, splits), _rag(logits, splits)])
    n, a = _rag(nodes, splits), _rag(logits, splits)
    n.values.requires_grad_(True)
    a.values.requires_grad_(True)
    out = layer([n, a])
    assert tuple(out.shape) == (5, 12) == tuple(plain.shape)
    d_n, d_a = torch.autograd.grad(out, [n.values, a.values], _cuda(g))
    graph = torch.from_numpy(np.repeat(np.arange(6), np.diff(splits)))
    refs = []
    for dt in (F32, F64):
        tn, ta = torch.tensor(nodes, dtype=dt, requires_grad=True), torch.tensor(logits, dtype=dt, requires_grad=True)
        o = aref.attention_pool(tn, ta, graph, 5)
        refs.append([o.detach().numpy()] + [v.numpy() for v in torch.autograd.grad(o, [tn, ta], torch.tensor(g, dtype=dt))])
    assert_rows_close(plain.cpu().numpy(), refs[0][0], refs[1][0], what="attention pooling")
    assert_rows_close(out.detach().cpu().numpy(), refs[0][0], refs[1][0], what="attention pooling on a tape")
    assert_rows_close(d_n.cpu().numpy(), refs[0][1], refs[1][1], what="attention pooling, node reverse")
    assert_rows_close(d_a.cpu().numpy(), refs[0][2], refs[1][2], what="attention pooling, logit reverse")


# ------------------------------------------------------------------------------------------------ layers
SIZES = (70, 1, 0, 21)


def _mol_batch(sizes=SIZES, seed=3, fn=20, fe=6, embed=False):
    """Bond graphs of these sizes (a random tree plus two ring bonds, both directions, sorted by receiver and sender);
    ``x`` / ``e``: float features, or float32 type numbers for the embedding inputs."""
    rng = np.random.default_rng(seed)
    graphs = []
    for n in sizes:
        bonds = {(int(rng.integers(0, a)), a) for a in range(1, n)}
        for _ in range(2 if n > 3 else 0):
            a, b = (int(v) for v in rng.choice(n, size=2, replace=False))
            bonds.add((min(a, b), max(a, b)))
        directed = sorted([(a, b) for a, b in bonds] + [(b, a) for a, b in bonds])
        graphs.append((n, np.array(directed, dtype=np.int64).reshape(-1, 2)))
    b = topo.batch(graphs)
    n, m = int(b["row_splits"][-1]), len(b["flat"])
    if embed:
        b["x"], b["e"] = rng.integers(0, 95, size=n).astype(np.float32), rng.integers(0, 5, size=m).astype(np.float32)
    else:
        b["x"], b["e"] = rng.normal(size=(n, fn)).astype(np.float32), rng.normal(size=(m, fe)).astype(np.float32)
    b["embedded"] = embed
    return b


def _inputs(b):
    return [_rag(b["x"], b["row_splits"]), _rag(b["e"], b["index_splits"]), _rag(b["indices"], b["index_splits"])]


def _both_routes(layer, inputs):
    """(fused result, fused launches, layer-sequence result, layer-sequence launches) of one layer call."""
    with torch.no_grad():
        layer.use_fused_attentive = True
        layer(inputs)                         # plans and CSRs are built once per batch
        count = _ffi.launch_count()
        fused = layer(inputs)
        fused_launches = _ffi.launch_count() - count
        layer.use_fused_attentive = False
        count = _ffi.launch_count()
        seq = layer(inputs)
        seq_launches = _ffi.launch_count() - count
        layer.use_fused_attentive = True
    return fused, fused_launches, seq, seq_launches


@pytest.mark.parametrize("use_edges,units", [(True, 32), (True, 64), (False, 32)])
def test_head_on_both_routes(use_edges, units):
    from gcnn_keras_amd.layers.conv.attentivefp_conv import AttentiveHeadFP
    b = _mol_batch()
    p = aref.head_params(np.random.default_rng(7), 20, units, 6 if use_edges else 0)
    layer = AttentiveHeadFP(units, use_edge_features=use_edges)
    inputs = _inputs(b)
    layer.ensure_built([(None, None, 20), (None, None, 6), (None, None, 2)])
    layer.set_weights(list(p.values()))
    fused, fused_launches, seq, seq_launches = _both_routes(layer, inputs)
    print("[attentivefp] head launches: fused %d, layer sequence %d" % (fused_launches, seq_launches))
    assert fused_launches == (5 if use_edges else 6) and fused_launches < seq_launches
    refs = [aref.head(torch.tensor(b["x"], dtype=dt), torch.tensor(b["e"], dtype=dt), b["flat"], aref.params_to(p, dt),
                      use_edges)[0].numpy() for dt in (F32, F64)]
    assert tuple(fused.values.shape) == (len(b["x"]), units)
    assert_rows_close(fused.values.cpu().numpy(), *refs, what="fused head")
    assert_rows_close(seq.values.cpu().numpy(), *refs, what="layer sequence head")
    # keyword arguments, and a tape, take the layer sequence
    with torch.no_grad():
        count = _ffi.launch_count()
        layer(inputs, training=False)
        assert _ffi.launch_count() - count == seq_launches
    inputs[0].values.requires_grad_(True)
    out = layer(inputs)
    assert out.values.requires_grad
    grad, = torch.autograd.grad(out.values.sum(), inputs[0].values)
    assert float(grad.abs().sum()) > 0.0


def test_heads_outside_the_served_sizes_take_the_layer_sequence():
    from gcnn_keras_amd.layers.conv.attentivefp_conv import AttentiveHeadFP
    b = _mol_batch(seed=5)
    for use_edges in (True, False):
        layer = AttentiveHeadFP(24, use_edge_features=use_edges)
        fused, fused_launches, seq, seq_launches = _both_routes(layer, _inputs(b))
        assert fused_launches == seq_launches and torch.equal(fused.values, seq.values)


# ------------------------------------------------------------------------------------------------ models
def _model_case(embed, output_embedding="graph", seed=21, units=32):
    """(model, inputs, batch, parameter dictionary): feature inputs of widths 12 / 6 or embedding inputs of 64 / 64."""
    from gcnn_keras_amd.literature import AttentiveFP
    fn, fe = (64, 64) if embed else (12, 6)
    b = _mol_batch(seed=seed, fn=fn, fe=fe, embed=embed)
    kwargs = dict(attention_args={"units": units}, output_embedding=output_embedding)
    if not embed:
        kwargs["inputs"] = [{"shape": (None, fn), "name": "node_attributes", "dtype": "float32", "ragged": True},
                            {"shape": (None, fe), "name": "edge_attributes", "dtype": "float32", "ragged": True},
                            {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True}]
    model = AttentiveFP.make_model(**kwargs)
    p = aref.model_params(np.random.default_rng(seed + 1), fn, fe, units, embed=(95, 5) if embed else None,
                          output_embedding=output_embedding)
    model.set_weights(list(p.values()))
    return model, _inputs(b), b, p


def _ref_forward(params, b, dt, output_embedding="graph"):
    x = torch.from_numpy(b["x"].astype(np.int64)) if b["embedded"] else torch.tensor(b["x"], dtype=dt)
    e = torch.from_numpy(b["e"].astype(np.int64)) if b["embedded"] else torch.tensor(b["e"], dtype=dt)
    return aref.model_forward(params, x, e, b["flat"], b["row_splits"], output_embedding=output_embedding)


def _model_refs(p, b, output_embedding="graph"):
    return [_ref_forward(aref.params_to(p, dt), b, dt, output_embedding).detach().numpy() for dt in (F32, F64)]


@pytest.mark.parametrize("embed,output_embedding", [(True, "graph"), (False, "graph"), (True, "node"), (False, "node")])
def test_model_on_both_routes(embed, output_embedding):
    model, x, b, p = _model_case(embed, output_embedding)
    assert model.fused_attentive_blocks == [True] * (3 if output_embedding == "graph" else 2)
    model.auto_graph = False
    with torch.no_grad():
        model(x)
        count = _ffi.launch_count()
        fused = model(x).cpu().numpy()
        fused_launches = _ffi.launch_count() - count
        model.use_fused_attentive = False
        count = _ffi.launch_count()
        seq = model(x).cpu().numpy()
        seq_launches = _ffi.launch_count() - count
        model.use_fused_attentive = True
    print("[attentivefp] launches per forward: fused %d, layer sequence %d" % (fused_launches, seq_launches))
    assert fused_launches < seq_launches
    r32, r64 = _model_refs(p, b, output_embedding)
    if output_embedding == "graph":
        assert fused.shape == (len(SIZES), 1)
    else:                                                         # the cast pads every graph to the longest
        assert fused.shape == (len(SIZES), max(SIZES), 1)
        rows = np.concatenate([np.arange(n) + g * max(SIZES) for g, n in enumerate(SIZES)])
        fused, seq = fused.reshape(-1, 1)[rows], seq.reshape(-1, 1)[rows]
    assert_rows_close(fused, r32, r64, what="model, fused")
    assert_rows_close(seq, r32, r64, what="model, layer sequence")


def test_graph_replay_stale_weights_and_the_switches():
    model, x, b, p = _model_case(True, seed=31)
    with torch.no_grad():
        first = model(x)
        assert model.last_route == "eager"
        second = model(x)
        assert model.last_route == "graph"                       # no host read-back: the forward captures
        third = model(x)
        assert model.last_route == "graph"
        assert torch.equal(first, second) and torch.equal(second, third)
    # weights changed in place: the replayed graph reads them where they are (the fused routes keep no repacked copy)
    model.set_weights([0.5 * w for w in model.get_weights()])
    with torch.no_grad():
        replayed = model(x)
        assert model.last_route == "graph"
        model.auto_graph = False
        eager = model(x)
        model.auto_graph = True
    assert torch.equal(replayed, eager) and not torch.equal(replayed, first)
    # re-bound inputs: another batch gets its own graph, the first one still replays
    other = _inputs(_mol_batch(seed=77, fn=64, fe=64, embed=True))
    with torch.no_grad():
        a = model(other)
        assert model.last_route == "eager"
        c = model(other)
        assert model.last_route == "graph" and torch.equal(a, c)
        again = model(x)
        assert model.last_route == "graph" and torch.equal(again, eager)
    # the model switch drops the captured graphs: the next call runs the layer sequence, not a replay of the fused route
    model.use_fused_attentive = False
    with torch.no_grad():
        seq = model(x)
    assert model.last_route == "eager"
    model.use_fused_attentive = True
    assert_rows_close(seq.cpu().numpy(), eager.cpu().numpy(), what="layer sequence after the switch")
    # a per-layer switch is part of a captured graph's identity too
    for lay in (model.attention_heads[0], model.readout):
        lay.use_fused_attentive = False
        with torch.no_grad():
            mixed = model(x)
        assert model.last_route == "eager" and model.use_fused_attentive is False
        lay.use_fused_attentive = True
        assert_rows_close(mixed.cpu().numpy(), eager.cpu().numpy(), what="one layer on the layer sequence")


def test_a_call_under_grad_takes_the_layer_sequence():
    model, x, b, p = _model_case(False, seed=35)
    with torch.no_grad():
        plain = model(x)
    model.requires_grad_(True)
    try:
        with torch.enable_grad():
            out = model(x)
            assert model.last_route == "eager" and out.requires_grad
            out.sum().backward()
        assert all(t.grad is not None for t in model.trainable_weights)
    finally:
        model.requires_grad_(False)
        for t in model.trainable_weights:
            t.grad = None
    assert_rows_close(out.detach().cpu().numpy(), plain.cpu().numpy(), what="on a tape vs fused")


# ------------------------------------------------------------------------------------------------ training
def _mse(pred, target):
    return torch.square(pred - target).mean(dim=-1).mean()


def _ref_trajectory(p, b, target, lr, steps, dt):
    w = [torch.tensor(a, dtype=dt, requires_grad=True) for a in p.values()]
    opt = torch.optim.SGD(w, lr=lr)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = _mse(_ref_forward(dict(zip(p.keys(), w)), b, dt), torch.from_numpy(target).to(dt))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses, [t.detach() for t in w]


def test_one_sgd_step_of_the_default_model():
    """Every weight of the default model (embedding inputs) after one step against the restatement's float64 step."""
    model, x, b, p = _model_case(True, seed=41)
    target = np.random.default_rng(4).uniform(0.0, 1.0, size=(len(SIZES), 1)).astype(np.float32)
    lr = 0.05
    model.compile(optimizer=torch.optim.SGD(model.trainable_weights, lr=lr), loss="mean_squared_error")
    loss = model.train_on_batch(x, target)
    assert not any(t.requires_grad for t in model.trainable_weights)
    after = model.get_weights()
    w = [torch.tensor(a, dtype=F64, requires_grad=True) for a in p.values()]
    ref = _mse(_ref_forward(dict(zip(p.keys(), w)), b, F64), torch.from_numpy(target).double())
    grads = torch.autograd.grad(ref, w)
    np.testing.assert_allclose(loss, float(ref.detach()), rtol=1e-5)
    names = [name for name, _ in model.weights]
    assert len(names) == len(p)
    for name, got, t0, g in zip(names, after, w, grads):
        want = (t0.detach() - lr * g).numpy()
        step = float(np.max(np.abs(lr * g.numpy())))
        # the gradient bar of the tests above (5e-5 of the tensor's largest step), plus two float32 ulps of the stored
        # weight (w - lr g is rounded once, and the float64 twin starts from the same float32 weight)
        assert np.max(np.abs(got - want)) <= 5e-5 * step + 2.4e-7 * float(np.max(np.abs(want))), name
        assert step > 0.0 or "embed" in name, name


def test_five_sgd_steps_and_the_fused_route_afterwards():
    model, x, b, p = _model_case(True, seed=43)
    target = np.random.default_rng(5).uniform(0.0, 1.0, size=(len(SIZES), 1)).astype(np.float32)
    lr = 0.05
    model.compile(optimizer=torch.optim.SGD(model.trainable_weights, lr=lr), loss="mean_squared_error")
    losses = [model.train_on_batch(x, target) for _ in range(5)]
    (r64, w64), (r32, _) = _ref_trajectory(p, b, target, lr, 5, F64), _ref_trajectory(p, b, target, lr, 5, F32)
    own = float(np.max(np.abs(np.array(r32) - np.array(r64)) / np.abs(np.array(r64))))
    rtol = 1e-5 if own <= 1e-5 else 2 * own
    print("[attentivefp] engine %s restatement %s (float32 restatement %.2e from float64, rtol %.1e)" % (
        losses, r64, own, rtol))
    np.testing.assert_allclose(losses, r64, rtol=rtol)
    assert len(set(losses)) == 5
    # the fused routes serve the trained weights
    trained = dict(zip(p.keys(), [t.numpy() for t in w64]))
    o32, o64 = _model_refs(trained, b)
    with torch.no_grad():
        count = _ffi.launch_count()
        after = model(x).cpu().numpy()
        fused_launches = _ffi.launch_count() - count
        model.use_fused_attentive = False
        count = _ffi.launch_count()
        seq = model(x).cpu().numpy()
        assert fused_launches < _ffi.launch_count() - count
        model.use_fused_attentive = True
    assert_rows_close(after, o32, o64, what="trained weights, fused")
    assert_rows_close(seq, o32, o64, what="trained weights, layer sequence")


def test_fit_under_binary_crossentropy():
    model, x, b, p = _model_case(True, seed=47)
    target = (np.random.default_rng(6).uniform(size=(len(SIZES), 1)) > 0.5).astype(np.float32)
    model.compile(optimizer=torch.optim.SGD(model.trainable_weights, lr=0.05), loss="binary_crossentropy")
    before = model.get_weights()
    history = model.fit(x, target, batch_size=2, epochs=1, shuffle=False)
    assert len(history.history["loss"]) == 1 and np.isfinite(history.history["loss"][0])
    assert any(not np.array_equal(a, c) for a, c in zip(before, model.get_weights()))
    # one step on graphs 0 and 1 alone: the loss is the restatement's binary cross-entropy on those rows
    w = aref.params_to(p, F64)
    prob = _ref_forward(w, b, F64)[:2].clamp(1e-7, 1 - 1e-7)
    t = torch.from_numpy(target[:2]).double()
    ref = float(-(t * torch.log(prob + 1e-7) + (1 - t) * torch.log(1 - prob + 1e-7)).mean(dim=-1).mean())
    model.set_weights(list(p.values()))
    loss = model.train_on_batch([r.take([0, 1]) for r in x], target[:2])
    np.testing.assert_allclose(loss, ref, rtol=1e-5)
