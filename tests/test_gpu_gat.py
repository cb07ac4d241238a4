"""GAT / GATv2 on csrc/mp_gat.hip: the kernel pair through the C ABI, the layers and the models on both routes, the reverse
rules of the attention pooling and training through the layer sequence, all against tests/gat_reference.py (float32 and
float64).  Index lists come from tests/topologies.py.

Bars: output rows through ``parity.assert_rows_close``; the logits are one float of cancelling terms per row and are held
as a tensor, ``max_rel(got, ref64) <= max(2e-6, 4 x max_rel(ref32, ref64))``; receivers without edges exactly 0."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import gat_reference as gref
import topologies as topo
from gcnn_keras_amd import _ffi, synth
from parity import assert_rows_close, max_rel

pytestmark = pytest.mark.gpu

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
    print("[gat] %s: logits %.2e of the tensor from float64 (float32 restatement %.2e)" % (what, err, e32))
    assert err <= max(2e-6, 4 * e32), what


# ------------------------------------------------------------------------------------------------ the kernels alone
@functools.lru_cache(maxsize=None)
def _kernel_case(name, v2):
    case = gref.kernel_case(v2, **gref.kernel_cases()[name])
    return case, gref.kernel_restate(case, torch.float32), gref.kernel_restate(case, torch.float64)


def _run_kernels(case):
    """Node-side products by ``dense_values`` on row-block views (GAT: ``mp_gat_node_scores_f32``), then the two entry
    points; ``(out, logits, perm0)``."""
    from gcnn_keras_amd.layers.modules import dense_values
    nodes = _rag(case["nodes"], case["row_splits"])
    idx = _rag(case["indices"], case["index_splits"])
    plan = idx.index_plan(nodes)
    plan.validate()
    ptr0, perm0, _ = plan.csr(0)
    n, e, u, d, v2 = plan.N, plan.M, case["u"], case["d"], case["v2"]
    f = case["nodes"].shape[1]
    hv, gv = nodes.values, _cuda(case["edges"])
    keep, cols = [], {k: [] for k in ("p", "q", "wc", "b", "a", "wn")}
    for p in case["heads"]:
        w = {k: _cuda(v) for k, v in p.items()}
        wn = dense_values(hv, w["linear_trafo/kernel"], w.get("linear_trafo/bias"), "linear")
        if v2:
            wa = w["alpha_activation/kernel"]
            pp, qq, wc = dense_values(hv, wa[:f], None), dense_values(hv, wa[f:2 * f], None), wa[2 * f:]
            bias, av = w.get("alpha_activation/bias"), w["alpha/kernel"]
        else:
            av = w["alpha/kernel"]
            pp, qq, wc, bias = None, None, av[2 * u:], None
        keep += [w, wn, pp, qq]
        for k, t in zip(("p", "q", "wc", "b", "a", "wn"), (pp, qq, wc if d else None, bias, av, wn)):
            cols[k].append(None if t is None else t.data_ptr())
    h = len(case["heads"])
    arr = lambda k: (ctypes.c_void_p * h)(*cols[k])
    code = _ffi.activation_code(case["act"])

    def once():
        out = torch.full((n, h, u), float("nan"), device="cuda")       # every row has to be written
        logits = torch.full((e, h), float("nan"), device="cuda")
        pq = None
        if not v2:
            pq = torch.full((n, h, 4), float("nan"), device="cuda")
            _ffi.call("mp_gat_node_scores_f32", h, u, arr("wn"), arr("a"), n, _ffi.ptr(pq), _ffi.stream())
        _ffi.call("mp_gat_logits_f32", _ffi.MP_GAT_V2 if v2 else _ffi.MP_GAT_V1, h, u, arr("p"), arr("q"), _ffi.ptr(pq),
                  arr("wc"), arr("b"), arr("a"), n, _ffi.ptr(gv) if d else None, d, _ffi.ptr(plan.cols), e, _ffi.ptr(perm0), code,
                  0.05, _ffi.ptr(logits), h, 0, _ffi.stream())
        _ffi.call("mp_gat_attend_f32", h, u, arr("wn"), n, _ffi.ptr(logits), h, 0, _ffi.ptr(plan.cols), e, _ffi.ptr(ptr0),
                  _ffi.ptr(perm0), _ffi.ptr(out), _ffi.stream())
        return out, logits

    first, again = once(), once()
    torch.cuda.synchronize()
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1]), "two runs differ"
    del keep
    return first[0].cpu().numpy(), first[1].cpu().numpy(), perm0


@pytest.mark.parametrize("v2", [False, True], ids=["gat", "gatv2"])
@pytest.mark.parametrize("name", sorted(gref.kernel_cases()))
def test_kernel_pair_against_the_restatement(name, v2):
    case, (o32, l32), (o64, l64) = _kernel_case(name, v2)
    out, logits, perm0 = _run_kernels(case)
    if "shuffled" in name:
        assert perm0 is not None
    elif "sorted" in name:
        assert perm0 is None
    n, h, u = o64.shape
    assert out.shape == o64.shape and logits.shape == l64.shape
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(logits))
    _logits_close(logits, l32, l64, name)
    assert_rows_close(out.reshape(n * h, u), o32.reshape(n * h, u), o64.reshape(n * h, u), what=name)
    lonely = topo.in_degrees(case["flat"], case["rows"]) == 0
    assert np.all(out[lonely] == 0.0) and (lonely.any() or name.startswith("exact"))


# ------------------------------------------------------------------------------------------------ layers
def _layer_batch(seed=3, f=20, fe=6):
    b = topo.batch(topo.with_empty_graphs([(90, topo.hub_edges(90, topo.SMALL_DEGREES, seed, True, True, "shuffled")),
                                           (3, topo.all_pairs(3))]))
    rng = np.random.default_rng(seed + 50)
    n, m = int(b["row_splits"][-1]), len(b["flat"])
    b.update(x=rng.normal(size=(n, f)).astype(np.float32), e=rng.normal(size=(m, fe)).astype(np.float32))
    return b


def _inputs(b):
    return [_rag(b["x"], b["row_splits"]), _rag(b["e"], b["index_splits"]), _rag(b["indices"], b["index_splits"])]


def _both_routes(layer, inputs):
    """(fused result, fused launches, layer-sequence result, layer-sequence launches) of one layer call."""
    with torch.no_grad():
        layer.use_fused_attention = True
        layer(inputs)                         # plans and CSRs are built once per batch
        count = _ffi.launch_count()
        fused = layer(inputs)
        fused_launches = _ffi.launch_count() - count
        layer.use_fused_attention = False
        count = _ffi.launch_count()
        seq = layer(inputs)
        seq_launches = _ffi.launch_count() - count
        layer.use_fused_attention = True
    return fused, fused_launches, seq, seq_launches


@pytest.mark.parametrize("v2", [False, True], ids=["gat", "gatv2"])
@pytest.mark.parametrize("use_edges,final", [(True, True), (False, False)])
def test_single_head_on_both_routes(v2, use_edges, final):
    from gcnn_keras_amd.layers.conv.gat_conv import AttentionHeadGAT, AttentionHeadGATV2
    b = _layer_batch()
    p = gref.head_params(np.random.default_rng(7), 20, 32, 6 if use_edges else 0, v2)
    layer = (AttentionHeadGATV2 if v2 else AttentionHeadGAT)(32, use_edge_features=use_edges, use_final_activation=final)
    inputs = _inputs(b)
    layer(inputs)
    layer.set_weights(list(p.values()))
    fused, fused_launches, seq, seq_launches = _both_routes(layer, inputs)
    assert fused_launches < seq_launches
    refs = [gref.head(torch.tensor(b["x"], dtype=dt), torch.tensor(b["e"], dtype=dt), b["flat"], gref.params_to(p, dt), v2,
                      use_edge_features=use_edges, use_final_activation=final)[0].numpy()
            for dt in (torch.float32, torch.float64)]
    assert tuple(fused.values.shape) == (len(b["x"]), 32)
    assert_rows_close(fused.values.cpu().numpy(), *refs, what="fused head")
    assert_rows_close(seq.values.cpu().numpy(), *refs, what="layer sequence head")


@pytest.mark.parametrize("v2", [False, True], ids=["gat", "gatv2"])
def test_heads_outside_the_served_sizes_take_the_layer_sequence(v2):
    from gcnn_keras_amd.layers.conv.gat_conv import AttentionHeadGAT, AttentionHeadGATV2
    b = _layer_batch(seed=5)
    layer = (AttentionHeadGATV2 if v2 else AttentionHeadGAT)(24, use_edge_features=True)
    fused, fused_launches, seq, seq_launches = _both_routes(layer, _inputs(b))
    assert fused_launches == seq_launches and torch.equal(fused.values, seq.values)


@pytest.mark.parametrize("heads,concat", [(4, True), (4, False), (9, True), (9, False)])
def test_multi_head_layer_on_both_routes(heads, concat):
    from gcnn_keras_amd.layers.conv.gat_conv import MultiHeadGATV2Layer
    b = _layer_batch(seed=9)
    rng = np.random.default_rng(10)
    ps = [gref.head_params(rng, 20, 32, 6, True) for _ in range(heads)]
    layer = MultiHeadGATV2Layer(units=32, num_heads=heads, concat_heads=concat, use_edge_features=True)
    inputs = _inputs(b)
    layer(inputs)
    layer.set_weights([a for p in ps for a in p.values()])
    (fh, fl), fused_launches, (sh, sl), seq_launches = _both_routes(layer, inputs)
    assert fused_launches < seq_launches
    m = len(b["flat"])
    assert tuple(fl.values.shape) == (m, heads, 1) and tuple(sl.values.shape) == (m, heads, 1)
    assert tuple(fh.values.shape) == (len(b["x"]), 32 * heads if concat else 32)
    refs = [gref.multi_head(torch.tensor(b["x"], dtype=dt), torch.tensor(b["e"], dtype=dt), b["flat"],
                            [gref.params_to(p, dt) for p in ps], concat=concat, use_edge_features=True)
            for dt in (torch.float32, torch.float64)]
    (h32, l32), (h64, l64) = [(h.numpy(), lg.numpy()) for h, lg in refs]
    for what, h, lg in (("fused", fh, fl), ("layer sequence", sh, sl)):
        assert_rows_close(h.values.cpu().numpy(), h32, h64, what="multi-head %s" % what)
        _logits_close(lg.values.cpu().numpy(), l32, l64, "multi-head %s" % what)


# ------------------------------------------------------------------------------------------------ models
UNITS, HEADS, DEPTH = 32, 5, 2


def _model_case(v2, concat, embed, seed=21, heads=HEADS):
    """(model, inputs, batch, parameter dictionary): feature inputs of widths 12 / 6 or embedding inputs of 64 / 64."""
    from gcnn_keras_amd.literature import GAT, GATv2
    b = synth.qm9_like_batch(num_graphs=6, seed=seed)
    rng = np.random.default_rng(seed + 1)
    n, m = int(b["node_splits"][-1]), int(b["edge_splits"][-1])
    b["flat"] = b["edge_indices"] + np.repeat(b["node_splits"][:-1], np.diff(b["edge_splits"]))[:, None]
    kwargs = dict(attention_args={"units": UNITS}, depth=DEPTH, attention_heads_num=heads, attention_heads_concat=concat)
    if embed:
        fn = fe = 64
        # the builder declares float32 numbers for embedding inputs (kgcnn/literature/GAT.py:24-26)
        b["x"], b["e"] = rng.integers(0, 95, size=n).astype(np.float32), rng.integers(0, 5, size=m).astype(np.float32)
        b["embedded"] = True
    else:
        fn, fe = 12, 6
        b["x"], b["e"] = rng.normal(size=(n, fn)).astype(np.float32), rng.normal(size=(m, fe)).astype(np.float32)
        kwargs["inputs"] = [{"shape": (None, fn), "name": "node_attributes", "dtype": "float32", "ragged": True},
                            {"shape": (None, fe), "name": "edge_attributes", "dtype": "float32", "ragged": True},
                            {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True}]
    model = (GATv2 if v2 else GAT).make_model(**kwargs)
    p = gref.model_params(rng, fn, fe, UNITS, heads, DEPTH, concat, v2, embed=(95, 5) if embed else None)
    model.set_weights(list(p.values()))
    x = [_rag(b["x"], b["node_splits"]), _rag(b["e"], b["edge_splits"]), _rag(b["edge_indices"], b["edge_splits"])]
    return model, x, b, p


def _model_refs(p, b, v2, concat, depth=DEPTH, heads=HEADS):
    out = []
    for dt in (torch.float32, torch.float64):
        x = torch.from_numpy(b["x"].astype(np.int64)) if b.get("embedded") else torch.tensor(b["x"], dtype=dt)
        e = torch.from_numpy(b["e"].astype(np.int64)) if b.get("embedded") else torch.tensor(b["e"], dtype=dt)
        out.append(gref.model_forward(gref.params_to(p, dt), x, e, b["flat"], b["node_splits"], depth=depth, heads=heads,
                                      concat=concat, v2=v2).detach().numpy())
    return out


@pytest.mark.parametrize("v2", [False, True], ids=["gat", "gatv2"])
@pytest.mark.parametrize("concat,embed", [(False, True), (True, False), (False, False), (True, True)])
def test_model_on_both_routes(v2, concat, embed):
    model, x, b, p = _model_case(v2, concat, embed)
    assert model.fused_attention_blocks == [True] * DEPTH
    model.auto_graph = False
    with torch.no_grad():
        model(x)
        count = _ffi.launch_count()
        fused = model(x).cpu().numpy()
        fused_launches = _ffi.launch_count() - count
        model.use_fused_attention = False
        count = _ffi.launch_count()
        seq = model(x).cpu().numpy()
        seq_launches = _ffi.launch_count() - count
        model.use_fused_attention = True
    print("[gat] launches per forward: fused %d, layer sequence %d" % (fused_launches, seq_launches))
    assert fused_launches < seq_launches
    r32, r64 = _model_refs(p, b, v2, concat)
    assert fused.shape == (6, 1)
    assert_rows_close(fused, r32, r64, what="model, fused")
    assert_rows_close(seq, r32, r64, what="model, layer sequence")


@pytest.mark.parametrize("v2", [False, True], ids=["gat", "gatv2"])
def test_graph_replay_stale_weights_and_the_switches(v2):
    model, x, b, p = _model_case(v2, False, True, seed=31)
    with torch.no_grad():
        first = model(x)
        assert model.last_route == "eager"
        second = model(x)
        assert model.last_route == "graph"
        third = model(x)
        assert model.last_route == "graph"
        assert torch.equal(first, second) and torch.equal(second, third)
    # weights changed in place: the replayed graph reads them where they are (the fused block keeps no repacked copy)
    model.set_weights([0.5 * w for w in model.get_weights()])
    with torch.no_grad():
        replayed = model(x)
        assert model.last_route == "graph"
        model.auto_graph = False
        eager = model(x)
        model.auto_graph = True
    assert torch.equal(replayed, eager) and not torch.equal(replayed, first)
    # the model switch drops the captured graphs: the next call runs the layer sequence, not a replay of the fused route
    model.use_fused_attention = False
    with torch.no_grad():
        seq = model(x)
    assert model.last_route == "eager"
    model.use_fused_attention = True
    assert_rows_close(seq.cpu().numpy(), eager.cpu().numpy(), what="layer sequence after the switch")
    # a per-head switch is part of a captured graph's identity too
    model.attention_heads[HEADS + 1].use_fused_attention = False
    with torch.no_grad():
        mixed = model(x)
    assert model.last_route == "eager" and model.use_fused_attention is False
    model.attention_heads[HEADS + 1].use_fused_attention = True
    assert_rows_close(mixed.cpu().numpy(), eager.cpu().numpy(), what="one head on the layer sequence")


# ------------------------------------------------------------------------------------------------ reverse rules alone
def _segments(seed=4):
    b = topo.batch(topo.with_empty_graphs([(40, topo.hub_edges(40, topo.SMALL_DEGREES, seed, order="shuffled")),
                                           (3, topo.all_pairs(3))]))
    nodes = _rag(np.zeros((int(b["row_splits"][-1]), 1), np.float32), b["row_splits"])
    idx = _rag(b["indices"], b["index_splits"])
    plan = idx.index_plan(nodes)
    ptr, perm, _ = plan.csr(0)
    assert perm is not None
    return b, plan, ptr, perm


@pytest.mark.parametrize("elems", [1, 4])
def test_segment_softmax_reverse(elems):
    from gcnn_keras_amd.ops.segment import segment_softmax_csr
    b, plan, ptr, perm = _segments()
    rng = np.random.default_rng(elems)
    m, n = len(b["flat"]), plan.N
    # unit-scale logits: y (g - sum y g) cancels where one edge dominates its segment, and with logits three times as
    # wide the float32 restatement itself is 1.2e-4 of a row from float64 (20 seeds; 4.9e-6 at unit scale)
    a, g = rng.normal(size=(m, elems)).astype(np.float32), rng.normal(size=(m, elems)).astype(np.float32)
    plain = segment_softmax_csr(_cuda(a), ptr, perm, n)
    leaf = _cuda(a).requires_grad_(True)
    y = segment_softmax_csr(leaf, ptr, perm, n)
    assert torch.equal(y.detach(), plain)                       # the tape does not change the forward's bits
    grad, = torch.autograd.grad(y, leaf, _cuda(g))
    refs = []
    for dt in (torch.float32, torch.float64):
        t = torch.tensor(a, dtype=dt, requires_grad=True)
        out = gref.segment_softmax(t, torch.from_numpy(b["flat"][:, 0]), n)
        refs.append((out.detach().numpy(), torch.autograd.grad(out, t, torch.tensor(g, dtype=dt))[0].numpy()))
    assert_rows_close(plain.cpu().numpy(), refs[0][0], refs[1][0], what="segment softmax")
    assert_rows_close(grad.cpu().numpy(), refs[0][1], refs[1][1], what="segment softmax reverse")


@pytest.mark.parametrize("elems", [1, 4])
def test_weighted_segment_sum_reverse(elems):
    from gcnn_keras_amd.ops.segment import segment_reduce_csr
    b, plan, ptr, perm = _segments(seed=6)
    rng = np.random.default_rng(10 + elems)
    m, n = len(b["flat"]), plan.N
    data, w = rng.normal(size=(m, elems)).astype(np.float32), rng.uniform(0.1, 1.0, size=(m, 1)).astype(np.float32)
    g = rng.normal(size=(n, elems)).astype(np.float32)
    seg = plan.col(0)
    plain = segment_reduce_csr(_ffi.MP_SUM, _cuda(data), ptr, perm, n, weight=_cuda(w))
    d_leaf, w_leaf = _cuda(data).requires_grad_(True), _cuda(w).requires_grad_(True)
    out = segment_reduce_csr(_ffi.MP_SUM, d_leaf, ptr, perm, n, weight=w_leaf, seg_ids=seg)
    assert torch.equal(out.detach(), plain)
    d_bar, w_bar = torch.autograd.grad(out, [d_leaf, w_leaf], _cuda(g))
    assert tuple(w_bar.shape) == (m, 1)
    # the weight alone on the tape, and the data alone (SegmentSum as before)
    w_only, = torch.autograd.grad(segment_reduce_csr(_ffi.MP_SUM, _cuda(data), ptr, perm, n, weight=w_leaf, seg_ids=seg),
                                  w_leaf, _cuda(g))
    d_only, = torch.autograd.grad(segment_reduce_csr(_ffi.MP_SUM, d_leaf, ptr, perm, n, weight=_cuda(w), seg_ids=seg),
                                  d_leaf, _cuda(g))
    assert torch.equal(w_only, w_bar) and torch.equal(d_only, d_bar)
    refs = []
    recv = torch.from_numpy(b["flat"][:, 0])
    for dt in (torch.float32, torch.float64):
        td, tw = torch.tensor(data, dtype=dt, requires_grad=True), torch.tensor(w, dtype=dt, requires_grad=True)
        o = torch.zeros((n, elems), dtype=dt).index_add(0, recv, tw * td)
        refs.append([o.detach().numpy()] + [t.numpy() for t in torch.autograd.grad(o, [td, tw], torch.tensor(g, dtype=dt))])
    assert_rows_close(plain.cpu().numpy(), refs[0][0], refs[1][0], what="weighted sum")
    assert_rows_close(d_bar.cpu().numpy(), refs[0][1], refs[1][1], what="weighted sum, data reverse")
    assert_rows_close(w_bar.cpu().numpy(), refs[0][2], refs[1][2], what="weighted sum, weight reverse")


# ------------------------------------------------------------------------------------------------ training
def _mse(pred, target):
    return torch.square(pred - target).mean(dim=-1).mean()


def _ref_forward(w, p, b, v2, heads, dt):
    params = dict(zip(p.keys(), w))
    x, e = torch.tensor(b["x"], dtype=dt), torch.tensor(b["e"], dtype=dt)
    return gref.model_forward(params, x, e, b["flat"], b["node_splits"], depth=2, heads=heads, concat=False, v2=v2)


def _train_case(v2, seed=41):
    """Depth 2, three averaged heads, feature inputs (no embedding tables among the weights)."""
    return _model_case(v2, False, False, seed=seed, heads=3)


@pytest.mark.parametrize("v2", [False, True], ids=["gat", "gatv2"])
def test_weight_gradients_match_restatement_autograd(v2):
    model, x, b, p = _train_case(v2)
    target = np.random.default_rng(4).uniform(0.0, 1.0, size=(6, 1)).astype(np.float32)
    model.requires_grad_(True)
    try:
        with torch.enable_grad():
            loss = _mse(model(x), _cuda(target))
            loss.backward()
        grads = [None if t.grad is None else t.grad.detach().cpu().numpy() for t in model.trainable_weights]
    finally:
        model.requires_grad_(False)
        for t in model.trainable_weights:
            t.grad = None
    refs = {}
    for dt in (torch.float32, torch.float64):
        w = [torch.tensor(a, dtype=dt, requires_grad=True) for a in p.values()]
        rl = _mse(_ref_forward(w, p, b, v2, 3, dt), torch.from_numpy(target).to(dt))
        refs[dt] = (float(rl.detach()), [g.numpy() for g in torch.autograd.grad(rl, w)])
    np.testing.assert_allclose(float(loss.detach()), refs[torch.float64][0], rtol=1e-5)
    names = [name for name, _ in model.weights]
    assert len(names) == len(p)
    for name, g, g32, g64 in zip(names, grads, refs[torch.float32][1], refs[torch.float64][1]):
        assert g is not None, name
        scale = max(float(np.max(np.abs(g64))), 1e-3)
        e32 = float(np.max(np.abs(g32 - g64))) / scale
        err = float(np.max(np.abs(g - g64))) / scale
        print("[training] %s: gradient %.2e of its scale from float64 (float32 restatement %.2e)" % (name, err, e32))
        assert err <= max(1e-5, min(4 * e32, 5e-5)), name
        if np.max(np.abs(g64)) > 0:
            assert np.max(np.abs(g)) > 0, name


@pytest.mark.parametrize("v2", [False, True], ids=["gat", "gatv2"])
def test_sgd_trajectory_fit_and_the_fused_route_afterwards(v2):
    model, x, b, p = _train_case(v2, seed=43)
    target = np.random.default_rng(5).uniform(0.0, 1.0, size=(6, 1)).astype(np.float32)
    lr = 0.05
    model.compile(optimizer=torch.optim.SGD(model.trainable_weights, lr=lr), loss="mean_squared_error")
    losses = [model.train_on_batch(x, target) for _ in range(5)]
    assert not any(t.requires_grad for t in model.trainable_weights)
    trajectories = {}
    for dt in (torch.float32, torch.float64):
        w = [torch.tensor(a, dtype=dt, requires_grad=True) for a in p.values()]
        opt = torch.optim.SGD(w, lr=lr)
        ref_losses = []
        for _ in range(5):
            opt.zero_grad()
            loss = _mse(_ref_forward(w, p, b, v2, 3, dt), torch.from_numpy(target).to(dt))
            loss.backward()
            opt.step()
            ref_losses.append(float(loss.detach()))
        trajectories[dt] = (ref_losses, [t.detach() for t in w])
    r64, r32 = np.array(trajectories[torch.float64][0]), np.array(trajectories[torch.float32][0])
    own = float(np.max(np.abs(r32 - r64) / np.abs(r64)))
    rtol = 1e-5 if own <= 1e-5 else 2 * own
    print("[training] engine %s restatement %s (float32 restatement %.2e from float64, rtol %.1e)" % (
        losses, list(r64), own, rtol))
    np.testing.assert_allclose(losses, r64, rtol=rtol)
    assert len(set(losses)) == 5
    # the fused route serves the trained weights
    trained = dict(zip(p.keys(), [t.numpy() for t in trajectories[torch.float64][1]]))
    o32, o64 = _model_refs(trained, b, v2, False, heads=3)
    with torch.no_grad():
        count = _ffi.launch_count()
        after = model(x).cpu().numpy()
        fused_launches = _ffi.launch_count() - count
        model.use_fused_attention = False
        count = _ffi.launch_count()
        seq = model(x).cpu().numpy()
        assert fused_launches < _ffi.launch_count() - count
        model.use_fused_attention = True
    assert_rows_close(after, o32, o64, what="trained weights, fused")
    assert_rows_close(seq, o32, o64, what="trained weights, layer sequence")
    history = model.fit(x, target, batch_size=2, epochs=2, seed=1)
    assert len(history.history["loss"]) == 2 and all(np.isfinite(v) for v in history.history["loss"])


@pytest.mark.parametrize("v2", [False, True], ids=["gat", "gatv2"])
def test_one_step_under_binary_crossentropy(v2):
    model, x, b, p = _train_case(v2, seed=47)
    target = (np.random.default_rng(6).uniform(size=(6, 1)) > 0.5).astype(np.float32)
    lr = 0.05
    model.compile(optimizer=torch.optim.SGD(model.trainable_weights, lr=lr), loss="binary_crossentropy")
    loss = model.train_on_batch(x, target)
    after = model.get_weights()
    w = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in p.values()]
    prob = _ref_forward(w, p, b, v2, 3, torch.float64).clamp(1e-7, 1 - 1e-7)
    t = torch.from_numpy(target).double()
    ref = -(t * torch.log(prob + 1e-7) + (1 - t) * torch.log(1 - prob + 1e-7)).mean(dim=-1).mean()
    grads = torch.autograd.grad(ref, w)
    np.testing.assert_allclose(loss, float(ref.detach()), rtol=1e-5)
    for (name, _), got, t0, g in zip(model.weights, after, w, grads):
        want = (t0.detach() - lr * g).numpy()
        step = float(np.max(np.abs(lr * g.numpy())))
        # the update to the gradient bar of the test above (5e-5 of the tensor's largest step), plus two float32 ulps of
        # the stored weight (w - lr g is rounded once, and the float64 twin starts from the same float32 weight)
        assert np.max(np.abs(got - want)) <= 5e-5 * step + 2.4e-7 * float(np.max(np.abs(want))), name
