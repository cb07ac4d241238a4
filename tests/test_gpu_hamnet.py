"""HamNet on the GPU: the message step's two kernels and the fingerprint kernel through the C ABI, both routes of the
layers and the model, graph replay, launch counts and training against the torch restatement (tests/hamnet_reference.py)
in float32 with its float64 twin.  Rows are compared through ``parity.assert_rows_close`` with its default bars; every
kernel output is pre-filled with NaN and every kernel case runs twice and has to give equal bits."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import hamnet_reference as href
import topologies as topo
from gcnn_keras_amd import _ffi
from parity import assert_rows_close, max_rel

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
NAN = float("nan")


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
    print("[hamnet] %s: logits %.2e of the tensor from float64 (float32 restatement %.2e)" % (what, err, e32))
    assert err <= max(2e-6, 4 * e32), what


# ------------------------------------------------------------------------------------------------ message kernels
@functools.lru_cache(maxsize=None)
def _message_case(name):
    case = href.message_case(**href.message_cases()[name])
    return case, href.message_restate(case, F32), href.message_restate(case, F64)


def _run_message_kernels(case):
    """Node-side products by ``dense_values`` on row-block views, then the two entry points, with and without the edge
    update; ``(mv, me in edge order, logits in edge order, perm0)``."""
    from gcnn_keras_amd.layers.modules import dense_values
    nodes = _rag(case["nodes"], case["row_splits"])
    idx = _rag(case["indices"], case["index_splits"])
    plan = idx.index_plan(nodes)
    plan.validate()
    ptr0, perm0, _ = plan.csr(0)
    n, e, f, u, ue, d, c = plan.N, plan.M, case["f"], case["u"], case["ue"], case["d"], case["c"]
    hv, gv, pv, qv = nodes.values, _cuda(case["edges"]), _cuda(case["p"]), _cuda(case["q"])
    w = {k: _cuda(v) for k, v in case["params"].items()}
    we = w["edge/kernel"]
    t = dense_values(hv, w["attend/kernel"], w.get("attend/bias"), case["act"])
    a, b = dense_values(hv, we[:f], None), dense_values(hv, we[f + 2 * c:], None)
    act, last = _ffi.activation_code(case["act"]), _ffi.activation_code(case["act_last"])

    def once(with_me):
        logit = torch.full((e,), NAN, device="cuda")                    # every entry has to be written
        me = torch.full((e, ue), NAN, device="cuda") if with_me else None
        mv = torch.full((n, u), NAN, device="cuda")
        _ffi.call("mp_hamnet_edge_f32", _ffi.ptr(a if with_me else None), _ffi.ptr(b if with_me else None), n, ue,
                  _ffi.ptr(pv), _ffi.ptr(qv), c, _ffi.ptr(gv), d, _ffi.ptr(w["align/kernel"]), _ffi.ptr(w.get("align/bias")),
                  _ffi.ptr(we[f:f + 2 * c] if with_me else None), _ffi.ptr(w.get("edge/bias") if with_me else None),
                  _ffi.ptr(plan.cols), e, _ffi.ptr(perm0), act, 0.05, _ffi.ptr(logit), _ffi.ptr(me), _ffi.stream())
        _ffi.call("mp_hamnet_attend_f32", u, _ffi.ptr(t), _ffi.ptr(logit), n, _ffi.ptr(plan.cols), e, _ffi.ptr(ptr0),
                  _ffi.ptr(perm0), last, 0.05, _ffi.ptr(mv), _ffi.stream())
        return [mv, logit] + ([me] if with_me else [])

    first, again, bare = once(True), once(True), once(False)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(first, again)), "two runs differ"
    assert torch.equal(first[0], bare[0]) and torch.equal(first[1], bare[1]), "the call without me gives other bits"
    by_position = first[1].cpu().numpy()
    logits = np.empty_like(by_position)
    logits[perm0.cpu().numpy() if perm0 is not None else np.arange(e)] = by_position
    return first[0].cpu().numpy(), first[2].cpu().numpy(), logits, perm0


@pytest.mark.parametrize("name", sorted(href.message_cases()))
def test_message_kernels_against_the_restatement(name):
    case, (mv32, me32, l32), (mv64, me64, l64) = _message_case(name)
    mv, me, logits, perm0 = _run_message_kernels(case)
    if "shuffled" in name:
        assert perm0 is not None
    elif "sorted" in name:
        assert perm0 is None
    assert mv.shape == mv64.shape and me.shape == me64.shape and logits.shape == l64.shape
    assert np.all(np.isfinite(mv)) and np.all(np.isfinite(me)) and np.all(np.isfinite(logits))
    if name.startswith("x80"):
        assert 80.0 <= np.abs(l64).max() <= 100.0          # the case is what its name says
    _logits_close(logits, l32, l64, name)
    assert_rows_close(mv, mv32, mv64, what=name + ", node update")
    if me.size:
        assert_rows_close(me, me32, me64, what=name + ", edge update")
    lonely = topo.in_degrees(case["flat"], case["rows"]) == 0
    assert lonely.any() and np.all(mv[lonely] == 0.0)      # act_last(0) = 0 for elu and linear


def test_message_entry_points_reject_bad_sizes_and_need_no_device_for_nothing():
    z = None                                                 # the sizes are refused first; the message says which
    edge = lambda ue=8, c=3, d=8, n=4, e=4: _ffi.call(
        "mp_hamnet_edge_f32", z, z, n, ue, z, z, c, z, d, z, None, z, None, z, e, None, 0, 0.05, z, z, _ffi.stream())
    attend = lambda u=8, n=4, e=4: _ffi.call("mp_hamnet_attend_f32", u, z, z, n, z, e, z, None, 0, 0.05, z, _ffi.stream())
    sizes = "multiple of 4|coordinates|bad sizes"
    for bad in (dict(ue=0), dict(ue=6), dict(ue=260), dict(c=0), dict(c=9), dict(d=0), dict(d=6), dict(d=260), dict(n=-1)):
        with pytest.raises(ValueError, match=sizes):
            edge(**bad)
    for bad in (dict(u=0), dict(u=6), dict(u=260), dict(e=-1)):
        with pytest.raises(ValueError, match=sizes):
            attend(**bad)
    with pytest.raises(ValueError, match="null pointer"):
        edge()
    _ffi.call("mp_hamnet_edge_f32", None, None, 4, 8, None, None, 3, None, 8, None, None, None, None, None, 0, None, 0, 0.05,
              None, None, None)                              # E = 0
    _ffi.call("mp_hamnet_attend_f32", 8, None, None, 0, None, 0, None, None, 0, 0.05, None, None)   # N = 0


# ------------------------------------------------------------------------------------------------ fingerprint kernel
@functools.lru_cache(maxsize=None)
def _fingerprint_case(name):
    case = href.fingerprint_case(**href.fingerprint_cases()[name])
    g = len(case["row_splits"]) - 1                          # the kernel serves every graph, trailing empty ones too
    return case, href.fingerprint_restate(case, F32, rows=g), href.fingerprint_restate(case, F64, rows=g)


def _fingerprint_call(vals, splits, g, w, case, out, term, stream=True):
    from gcnn_keras_amd.layers.modules import dense_values
    from gcnn_keras_amd.ops.segment import reduce_op_code
    n, depth, act = int(vals.shape[0]), case["depth"], case["act"]
    m = dense_values(vals, w["v2m/kernel"], w.get("v2m/bias"), act) if n > 0 else None
    keep, cols = [m], {key: [] for key in ("T", "w", "b", "K", "R", "b_in", "b_rec")}
    for i in range(depth):
        bias = w.get("g%d/bias" % i)
        row = {"T": dense_values(vals, w["r%d/attend/kernel" % i], w.get("r%d/attend/bias" % i), act) if n > 0 else None,
               "w": w["r%d/align/kernel" % i], "b": w.get("r%d/align/bias" % i), "K": w["g%d/kernel" % i],
               "R": w["g%d/recurrent_kernel" % i], "b_in": None if bias is None else bias[0],
               "b_rec": None if bias is None else bias[1]}
        keep.append(row)                                     # held: a pointer alone keeps no tensor alive
        for key, tensor in row.items():
            cols[key].append(None if tensor is None else tensor.data_ptr())
    arr = lambda key: (ctypes.c_void_p * max(depth, 1))(*cols[key])
    _ffi.call("mp_hamnet_fingerprint_f32", _ffi.ptr(vals), _ffi.ptr(m), n, _ffi.ptr(splits), g, case["f"], case["u"],
              case["ua"], depth, reduce_op_code(case["pooling_method"]), arr("T"), arr("w"), arr("b"), arr("K"), arr("R"),
              arr("b_in"), arr("b_rec"), _ffi.activation_code(act), 0.05, _ffi.activation_code("elu"),
              _ffi.activation_code("tanh"), _ffi.activation_code("sigmoid"), _ffi.ptr(term), _ffi.ptr(out), _ffi.stream())
    return keep


def _run_fingerprint(case):
    vals, splits = _cuda(case["nodes"]), _cuda(case["row_splits"])
    g = len(case["row_splits"]) - 1
    w = {k: _cuda(v) for k, v in case["params"].items()}

    def once():
        out = torch.full((g, case["u"]), NAN, device="cuda")                 # every row has to be written
        term = torch.full((max(len(case["nodes"]), 1),), NAN, dtype=torch.float64, device="cuda")
        _fingerprint_call(vals, splits, g, w, case, out, term)
        return out

    first, again = once(), once()
    torch.cuda.synchronize()
    assert torch.equal(first, again), "two runs differ"
    return first.cpu().numpy()


def _fingerprint_layer(case):
    from gcnn_keras_amd.layers.conv.hamnet_conv import HamNetFingerprintGenerator
    layer = HamNetFingerprintGenerator(case["u"], case["ua"], depth=case["depth"], pooling_method=case["pooling_method"],
                                       activation=case["act"], use_bias=case["bias"])
    layer.ensure_built((None, None, case["f"]))
    layer.set_weights(list(case["params"].values()))
    return layer


@pytest.mark.parametrize("name", sorted(href.fingerprint_cases()))
def test_fingerprint_kernel_against_the_restatement_and_the_layer_sequence(name):
    case, r32, r64 = _fingerprint_case(name)
    out = _run_fingerprint(case)
    assert out.shape == r64.shape and np.all(np.isfinite(out))
    assert_rows_close(out, r32, r64, what=name)
    rows = href.graph_rows(case["row_splits"])
    layer, x = _fingerprint_layer(case), _rag(case["nodes"], case["row_splits"])
    assert layer.fused_supported(case["f"])
    with torch.no_grad():
        count = _ffi.launch_count()
        fused = layer(x)
        fused_launches = _ffi.launch_count() - count
        layer.use_fused_hamnet = False
        count = _ffi.launch_count()
        seq = layer(x)
        seq_launches = _ffi.launch_count() - count
    assert tuple(fused.shape) == tuple(seq.shape) == (rows, case["u"])   # PoolingNodes' count: trailing empties dropped
    assert np.array_equal(fused.cpu().numpy(), out[:rows])               # the layer's fused route is this call
    assert fused_launches == 2 + case["depth"] and (fused_launches < seq_launches or case["depth"] == 0)
    assert_rows_close(seq.cpu().numpy(), r32[:rows], r64[:rows], what=name + ", layer sequence")


def test_fingerprint_entry_point_rejects_bad_sizes_and_needs_no_device_for_no_graphs():
    z = None                                                 # the sizes are refused first; the message says which
    call = lambda f=8, u=8, ua=8, depth=1, pool=_ffi.MP_SUM, g=1: _ffi.call(
        "mp_hamnet_fingerprint_f32", z, z, 1, z, g, f, u, ua, depth, pool, z, z, z, z, z, z, z, 0, 0.05, 0, 0, 0, z, z,
        _ffi.stream())
    for bad in (dict(f=0), dict(f=6), dict(f=260), dict(u=6), dict(u=260), dict(ua=0), dict(ua=260), dict(depth=9),
                dict(depth=-1), dict(pool=_ffi.MP_MAX), dict(g=-1)):
        with pytest.raises(ValueError, match="multiples of 4|depth must be|sum or mean|bad sizes"):
            call(**bad)
    with pytest.raises(ValueError, match="null pointer"):
        call()
    _ffi.call("mp_hamnet_fingerprint_f32", None, None, 0, None, 0, 8, 8, 8, 2, _ffi.MP_MEAN, None, None, None, None, None,
              None, None, 0, 0.05, 0, 0, 0, None, None, None)                # G = 0


# ------------------------------------------------------------------------------------------------ layers
F_NODE, F_EDGE, COORDS = 12, 8, 3


def _layer_inputs(b, seed=5):
    rng = np.random.default_rng(seed)
    pm = rng.normal(size=b["xyz"].shape).astype(np.float32)
    return [_rag(b["x"], b["row_splits"]), _rag(b["e"], b["index_splits"]), _rag(pm, b["row_splits"]),
            _rag(b["xyz"], b["row_splits"]), _rag(b["indices"], b["index_splits"])], pm


def _both_routes(layer, inputs):
    """(fused result, fused launches, layer-sequence result, layer-sequence launches) of one layer call."""
    with torch.no_grad():
        for flag in (False, True):            # plans and CSRs are built once per batch, on either route
            layer.use_fused_hamnet = flag
            layer(inputs)
        count = _ffi.launch_count()
        fused = layer(inputs)
        fused_launches = _ffi.launch_count() - count
        layer.use_fused_hamnet = False
        count = _ffi.launch_count()
        seq = layer(inputs)
        seq_launches = _ffi.launch_count() - count
        layer.use_fused_hamnet = True
    return fused, fused_launches, seq, seq_launches


@pytest.mark.parametrize("edge_update", [True, False], ids=["with-me", "without-me"])
def test_message_layer_on_both_routes(edge_update):
    from gcnn_keras_amd.layers.conv.hamnet_conv import HamNaiveDynMessage
    b = href.mol_batch(fn=F_NODE, fe=F_EDGE)
    assert len(b["sizes"]) == 19 and 0 in b["sizes"]
    p = href.message_params(np.random.default_rng(7), F_NODE, F_EDGE, COORDS, 36, 20)
    layer = HamNaiveDynMessage(36, 20)
    layer.return_edge_update = edge_update
    inputs, pm = _layer_inputs(b)
    layer.ensure_built([(None, None, F_NODE), (None, None, F_EDGE), (None, None, COORDS), (None, None, COORDS),
                        (None, None, 2)])
    layer.set_weights(list(p.values()))
    assert layer.fused_supported(F_NODE, F_EDGE, COORDS)
    fused, fused_launches, seq, seq_launches = _both_routes(layer, inputs)
    print("[hamnet] message launches: fused %d, layer sequence %d" % (fused_launches, seq_launches))
    assert fused_launches == (5 if edge_update else 3) and fused_launches < seq_launches
    refs = [href.message(*(torch.tensor(a, dtype=dt) for a in (b["x"], b["e"], pm, b["xyz"])), b["flat"],
                         href.params_to(p, dt)) for dt in (F32, F64)]
    assert_rows_close(fused[0].values.cpu().numpy(), refs[0][0].numpy(), refs[1][0].numpy(), what="fused, nodes")
    assert_rows_close(seq[0].values.cpu().numpy(), refs[0][0].numpy(), refs[1][0].numpy(), what="layer sequence, nodes")
    if edge_update:
        assert_rows_close(fused[1].values.cpu().numpy(), refs[0][1].numpy(), refs[1][1].numpy(), what="fused, edges")
        assert_rows_close(seq[1].values.cpu().numpy(), refs[0][1].numpy(), refs[1][1].numpy(), what="layer sequence, edges")
    else:
        assert fused[1] is None and seq[1] is None
    # keyword arguments, and a tape, take the layer sequence
    with torch.no_grad():
        count = _ffi.launch_count()
        layer(inputs, training=False)
        assert _ffi.launch_count() - count == seq_launches
    inputs[0].values.requires_grad_(True)
    out = layer(inputs)[0]
    assert out.values.requires_grad
    grad, = torch.autograd.grad(out.values.sum(), inputs[0].values)
    assert float(grad.abs().sum()) > 0.0


def test_message_layer_outside_the_served_sizes_takes_the_layer_sequence():
    from gcnn_keras_amd.layers.conv.hamnet_conv import HamNaiveDynMessage
    b = href.mol_batch(fn=F_NODE, fe=F_EDGE, seed=9)
    layer = HamNaiveDynMessage(30, 20)                       # units no multiple of 4
    inputs, _ = _layer_inputs(b)
    fused, fused_launches, seq, seq_launches = _both_routes(layer, inputs)
    assert fused_launches == seq_launches
    assert torch.equal(fused[0].values, seq[0].values) and torch.equal(fused[1].values, seq[1].values)


def test_fingerprint_layer_on_both_routes():
    from gcnn_keras_amd.layers.conv.hamnet_conv import HamNetFingerprintGenerator
    b = href.mol_batch(fn=F_NODE, fe=F_EDGE, sizes=href.MOL_SIZES + (0,))      # also a trailing empty graph
    p = href.fingerprint_params(np.random.default_rng(11), F_NODE, 16, 24, 3)
    layer = HamNetFingerprintGenerator(16, 24, depth=3)
    layer.ensure_built((None, None, F_NODE))
    layer.set_weights(list(p.values()))
    x = _rag(0.3 * b["x"], b["row_splits"])
    fused, fused_launches, seq, seq_launches = _both_routes(layer, x)
    print("[hamnet] fingerprint launches: fused %d, layer sequence %d" % (fused_launches, seq_launches))
    assert fused_launches == 5 and fused_launches < seq_launches
    refs = [href.fingerprint(torch.tensor(0.3 * b["x"], dtype=dt), b["row_splits"], href.params_to(p, dt), 3).numpy()
            for dt in (F32, F64)]
    assert tuple(fused.shape) == (19, 16)
    assert_rows_close(fused.cpu().numpy(), *refs, what="fused fingerprint")
    assert_rows_close(seq.cpu().numpy(), *refs, what="layer sequence fingerprint")
    with torch.no_grad():
        count = _ffi.launch_count()
        layer(x, training=False)                             # keyword arguments take the layer sequence
        assert _ffi.launch_count() - count == seq_launches
    layer_d = HamNetFingerprintGenerator(16, 24, depth=3, use_dropout=True, rate=0.5)
    layer_d.ensure_built((None, None, F_NODE))
    layer_d.set_weights(list(p.values()))
    with torch.no_grad():
        assert torch.equal(layer_d(x), fused)                # dropout outside training is the identity


def test_union_and_readout_layers_against_the_restatement():
    """The three layers without a launch of their own: the switch changes nothing, the restatement holds."""
    from gcnn_keras_amd.layers.conv.hamnet_conv import HamNetGlobalReadoutAttend, HamNetGRUUnion, HamNetNaiveUnion
    b = href.mol_batch(fn=F_NODE, fe=F_EDGE, seed=13)
    rng = np.random.default_rng(17)
    n = len(b["x"])
    xu = rng.normal(size=(n, 20)).astype(np.float32)
    x, u = _rag(b["x"], b["row_splits"]), _rag(xu, b["row_splits"])
    t = lambda a, dt: torch.tensor(a, dtype=dt)
    # naive union
    p = {}
    href._dense_params(p, rng, "dense", F_NODE + 20, 16, True)
    layer = HamNetNaiveUnion(16)
    layer.ensure_built([(None, None, F_NODE), (None, None, 20)])
    layer.set_weights(list(p.values()))
    fused, _, seq, _ = _both_routes(layer, [x, u])
    assert torch.equal(fused.values, seq.values)
    refs = [href.naive_union(t(b["x"], dt), t(xu, dt), href.params_to(p, dt)).numpy() for dt in (F32, F64)]
    assert_rows_close(fused.values.cpu().numpy(), *refs, what="naive union")
    # GRU union
    p = href.gru_params(rng, 20, F_NODE, "gru")
    layer = HamNetGRUUnion(F_NODE)
    layer.ensure_built([(None, None, F_NODE), (None, None, 20)])
    layer.set_weights(list(p.values()))
    with torch.no_grad():
        got = layer([x, u]).values.cpu().numpy()
    refs = [href.gru_cell(t(xu, dt), t(b["x"], dt), href.params_to(p, dt)).numpy() for dt in (F32, F64)]
    assert_rows_close(got, *refs, what="GRU union")
    # readout attend
    rows = href.graph_rows(b["row_splits"])
    state = rng.normal(size=(rows, 16)).astype(np.float32)
    p = {}
    href._dense_params(p, rng, "attend", F_NODE, 24, True)
    href._dense_params(p, rng, "align", 16 + F_NODE, 1, True)
    layer = HamNetGlobalReadoutAttend(24)
    layer.ensure_built([(None, 16), (None, None, F_NODE)])
    layer.set_weights(list(p.values()))
    fused, _, seq, _ = _both_routes(layer, [_cuda(state), x])
    assert torch.equal(fused[0], seq[0]) and torch.equal(fused[1].values, seq[1].values)
    graph = torch.from_numpy(np.repeat(np.arange(rows), np.diff(b["row_splits"])[:rows]))
    refs = [href.readout_attend(t(state, dt), t(b["x"], dt), graph, rows, href.params_to(p, dt)) for dt in (F32, F64)]
    assert_rows_close(fused[0].cpu().numpy(), refs[0][0].numpy(), refs[1][0].numpy(), what="readout attend")
    _logits_close(fused[1].values.cpu().numpy(), refs[0][1].numpy(), refs[1][1].numpy(), "readout attend")


# ------------------------------------------------------------------------------------------------ models
UNIONS = ("gru", "naive", "None")


def _model_case(union_node="gru", union_edge="None", depth=1, output_embedding="graph", seed=21):
    """(model, inputs, batch, parameter dictionary) of the reference's inputs: type numbers and coordinates."""
    from gcnn_keras_amd.literature import HamNet
    b = href.mol_batch(seed=seed, embed=True)
    model = HamNet.make_model(depth=depth, union_type_node=union_node, union_type_edge=union_edge,
                              output_embedding=output_embedding)
    p = href.model_params(np.random.default_rng(seed + 1), 64, 64, depth=depth, union_node=union_node,
                          union_edge=union_edge, output_embedding=output_embedding)
    model.set_weights(list(p.values()))
    x = [_rag(b["x"], b["row_splits"]), _rag(b["e"], b["index_splits"]), _rag(b["indices"], b["index_splits"]),
         _rag(b["xyz"], b["row_splits"])]
    return model, x, b, dict(p, _kw=dict(depth=depth, union_node=union_node, union_edge=union_edge,
                                         output_embedding=output_embedding))


def _ref_forward(params, b, dt, kw):
    x, e = torch.from_numpy(b["x"].astype(np.int64)), torch.from_numpy(b["e"].astype(np.int64))
    return href.model_forward(params, x, e, b["flat"], torch.tensor(b["xyz"], dtype=dt), b["row_splits"], **kw)


def _weights_of(p):
    return {k: v for k, v in p.items() if k != "_kw"}


def _model_refs(p, b):
    return [_ref_forward(href.params_to(_weights_of(p), dt), b, dt, p["_kw"]).detach().numpy() for dt in (F32, F64)]


def _routes_of_model(model, x):
    model.auto_graph = False
    with torch.no_grad():
        for flag in (False, True):            # plans and CSRs are built once per batch, on either route
            model.use_fused_hamnet = flag
            model(x)
        count = _ffi.launch_count()
        fused = model(x).cpu().numpy()
        fused_launches = _ffi.launch_count() - count
        model.use_fused_hamnet = False
        count = _ffi.launch_count()
        seq = model(x).cpu().numpy()
        seq_launches = _ffi.launch_count() - count
        model.use_fused_hamnet = True
    model.auto_graph = True
    return fused, fused_launches, seq, seq_launches


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("union_edge", UNIONS)
@pytest.mark.parametrize("union_node", UNIONS)
def test_model_on_both_routes(union_node, union_edge, depth):
    model, x, b, p = _model_case(union_node, union_edge, depth)
    assert model.fused_hamnet_blocks == [True] * (depth + 1)
    fused, fused_launches, seq, seq_launches = _routes_of_model(model, x)
    assert fused_launches < seq_launches
    r32, r64 = _model_refs(p, b)
    assert fused.shape == (len(b["sizes"]), 1)
    assert_rows_close(fused, r32, r64, what="model, fused")
    assert_rows_close(seq, r32, r64, what="model, layer sequence")


def test_node_output_on_both_routes():
    model, x, b, p = _model_case(output_embedding="node")
    fused, fused_launches, seq, seq_launches = _routes_of_model(model, x)
    assert fused_launches < seq_launches
    r32, r64 = _model_refs(p, b)
    sizes = b["sizes"]
    assert fused.shape == (len(sizes), max(sizes), 1)        # the cast pads every graph to the longest
    rows = np.concatenate([np.arange(n) + g * max(sizes) for g, n in enumerate(sizes)])
    assert_rows_close(fused.reshape(-1, 1)[rows], r32, r64, what="node output, fused")
    assert_rows_close(seq.reshape(-1, 1)[rows], r32, r64, what="node output, layer sequence")


def test_launch_counts_of_the_default_model():
    model, x, b, p = _model_case()
    _, fused_launches, _, seq_launches = _routes_of_model(model, x)
    print("[hamnet] engine calls per forward of the default model: fused %d, layer sequence %d"
          % (fused_launches, seq_launches))
    assert fused_launches < seq_launches


def test_graph_replay_on_one_stream():
    model, x, b, p = _model_case(seed=31)
    with torch.no_grad():
        first = model(x)
        assert model.last_route == "eager"
        second = model(x)
        assert model.last_route == "graph"                   # no host read-back: the forward captures
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
    # the model switch drops the captured graphs: the next call runs the layer sequence, not a replay of the fused route
    model.use_fused_hamnet = False
    with torch.no_grad():
        seq = model(x)
    assert model.last_route == "eager"
    model.use_fused_hamnet = True
    assert_rows_close(seq.cpu().numpy(), eager.cpu().numpy(), what="layer sequence after the switch")


# ------------------------------------------------------------------------------------------------ training
def _mse(pred, target):
    return torch.square(pred - target).mean(dim=-1).mean()


def _ref_trajectory(p, b, target, lr, steps, dt):
    names, kw = list(_weights_of(p)), p["_kw"]
    w = [torch.tensor(p[k], dtype=dt, requires_grad=True) for k in names]
    opt = torch.optim.SGD(w, lr=lr)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = _mse(_ref_forward(dict(zip(names, w)), b, dt, kw), torch.from_numpy(target).to(dt))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses, [t.detach() for t in w]


def test_two_sgd_steps_of_the_default_model(monkeypatch):
    model, x, b, p = _model_case(seed=41)
    target = np.random.default_rng(4).uniform(0.0, 1.0, size=(len(b["sizes"]), 1)).astype(np.float32)
    lr = 0.05
    model.compile(optimizer=torch.optim.SGD(model.trainable_weights, lr=lr), loss="mean_squared_error")
    before = model.get_weights()
    called, plain_call = [], _ffi.call
    monkeypatch.setattr(_ffi, "call", lambda name, *args: (called.append(name), plain_call(name, *args))[1])
    losses = [model.train_on_batch(x, target) for _ in range(2)]
    assert called and not [name for name in called if name.startswith("mp_hamnet")]   # a tape takes the layer sequence
    assert not any(t.requires_grad for t in model.trainable_weights)
    (r64, w64), (r32, _) = _ref_trajectory(p, b, target, lr, 2, F64), _ref_trajectory(p, b, target, lr, 2, F32)
    own = float(np.max(np.abs(np.array(r32) - np.array(r64)) / np.abs(np.array(r64))))
    rtol = 1e-5 if own <= 1e-5 else 2 * own
    print("[hamnet] engine %s restatement %s (float32 restatement %.2e from float64, rtol %.1e)" % (losses, r64, own, rtol))
    np.testing.assert_allclose(losses, r64, rtol=rtol)
    assert len(set(losses)) == 2
    # every weight moved, except the last round's edge update, which nobody reads (its gradient is zero in float64 too);
    # the bias of a logit is left out: the softmax does not see it, its gradient is zero up to rounding
    names, after = list(_weights_of(p)), model.get_weights()
    for name, a, c, t0, t1 in zip(names, before, after, _weights_of(p).values(), w64):
        if name.endswith("align/bias"):
            continue
        moved_in_float64 = not np.array_equal(t0.astype(np.float64), t1.numpy())
        assert moved_in_float64 == (not name.startswith("msg0/edge/")), name
        assert (not np.array_equal(a, c)) == moved_in_float64, name
    # the fused routes serve the trained weights
    trained = dict(zip(names, [t.numpy() for t in w64]), _kw=p["_kw"])
    o32, o64 = _model_refs(trained, b)
    del called[:]
    with torch.no_grad():
        model.auto_graph = False
        served = model(x).cpu().numpy()
    assert {"mp_hamnet_edge_f32", "mp_hamnet_attend_f32", "mp_hamnet_fingerprint_f32"} <= set(called)
    assert_rows_close(served, o32, o64, what="trained weights, fused")


def test_fit_runs_through_the_layer_sequence():
    model, x, b, p = _model_case(seed=47)
    target = np.random.default_rng(6).uniform(0.0, 1.0, size=(len(b["sizes"]), 1)).astype(np.float32)
    model.compile(optimizer="adam", loss="mean_absolute_error")
    before = model.get_weights()
    history = model.fit(x, target, batch_size=8, epochs=1, shuffle=False)
    assert len(history.history["loss"]) == 1 and np.isfinite(history.history["loss"][0])
    assert any(not np.array_equal(a, c) for a, c in zip(before, model.get_weights()))
