"""MAT on csrc/mp_mat.hip: the kernel alone through the C ABI on the edges of both tiles, its merge epilogue, the head
layer, and the model on both routes with graph replay, ``predict`` in batches, the route switch and the launch counts,
all against tests/mat_reference.py (float32 and float64; tests/test_mat_api.py shows that its padded form - the
reference's - and its per-molecule form are the same function).

Bars: ``parity.assert_rows_close`` with its defaults.  Outputs are prefilled with NaN, so a row the kernel does not write
shows; two calls and a call on a second stream give equal bits."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mat_reference as mref
from gcnn_keras_amd import _ffi
from parity import assert_rows_close

pytestmark = pytest.mark.gpu

R, S = _ffi.MP_MAT_RECV_TILE, _ffi.MP_MAT_SEND_TILE
TRAFO = {None: _ffi.MP_MAT_TRAFO_NONE, "exp": _ffi.MP_MAT_TRAFO_EXP, "softmax": _ffi.MP_MAT_TRAFO_SOFTMAX}


def _rag(values, splits):
    from gcnn_keras_amd.ragged import RaggedTensor
    return RaggedTensor.from_numpy(np.ascontiguousarray(values), splits)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _raw(t):
    return ctypes.c_void_p(t.data_ptr())


def test_the_restatement_knows_the_tiles():
    assert (mref.R, mref.S) == (R, S)


# ------------------------------------------------------------------------------------------------ the kernel alone
@functools.lru_cache(maxsize=None)
def _kernel_case(name):
    case = mref.kernel_case(**mref.kernel_cases()[name])
    return case, mref.kernel_restate(case, torch.float32).numpy(), mref.kernel_restate(case, torch.float64).numpy()


def _plan(case):
    nodes = _rag(np.zeros((int(case["node_splits"][-1]), 1), np.float32), case["node_splits"])
    idx = _rag(case["idx"], case["edge_splits"])
    plan = idx.index_plan(nodes)
    plan.validate()
    return plan, nodes.row_splits


def _device(case):
    return {key: _cuda(case[key]) for key in ("q", "k", "v", "xyz", "w")}


def _attend(case, plan, splits, dev, q=None, k=None, v=None, wm=None, e=0, merge=0, h=None, flags=None):
    """One ``mp_mat_attention_f32`` call on the current stream into an output prefilled with NaN."""
    q, k, v = (dev[n] if t is None else t for n, t in (("q", q), ("k", k), ("v", v)))
    n, c = int(case["node_splits"][-1]), case["heads"] * case["units"]
    ptr0, perm0, _ = plan.csr(0)
    out = torch.full((n, e if wm is not None else c), float("nan"), device="cuda")
    ld = lambda t: int(t.stride(0)) if n > 1 else c
    _ffi.call("mp_mat_attention_f32", _raw(q), ld(q), _raw(k), ld(k), _raw(v), ld(v), n, case["heads"], case["units"],
              _ffi.ptr(dev["xyz"]), _ffi.ptr(splits), len(case["node_splits"]) - 1, _ffi.ptr(ptr0), _ffi.ptr(perm0),
              _ffi.ptr(plan.col(1)), _ffi.ptr(dev["w"]), plan.M, TRAFO[case["trafo"]], case["la"], case["ld"], case["lg"],
              1 if case["add_identity"] else 0, _ffi.ptr(wm), e, merge, _ffi.ptr(h), _ffi.ptr(out), _ffi.ptr(flags),
              _ffi.stream())
    return out


@pytest.mark.parametrize("name", sorted(mref.kernel_cases()))
def test_kernel_against_the_restatement(name):
    case, r32, r64 = _kernel_case(name)
    plan, splits = _plan(case)
    dev = _device(case)
    first = _attend(case, plan, splits, dev)
    again = _attend(case, plan, splits, dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _attend(case, plan, splits, dev)
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(first, again), "two calls differ"
    assert torch.equal(first, other), "a second stream differs"
    _, perm0, _ = plan.csr(0)
    if case["edges"] in ("shuffled", "duplicates"):
        assert perm0 is not None
    elif case["edges"] in ("sorted", "loops"):
        assert perm0 is None
    got = first.cpu().numpy()
    assert got.shape == r64.shape and np.all(np.isfinite(got)), "a row was not written, or overflowed"
    assert_rows_close(got, r32, r64, what=name)
    assert int(plan.flags.item()) & _ffi.MP_FLAG_OOB == 0


def test_zero_q_is_the_mean_and_one_atom_is_itself():
    """With only the attention term: ``q = 0`` weighs every atom of the molecule equally, whatever ``k`` is, and a
    molecule of one atom returns its own ``v``."""
    case = dict(mref.kernel_case(sizes=(1, S + 3, 0, 5), heads=1, units=6, seed=21), la=1.0, ld=0.0, lg=0.0)
    case["q"] = np.zeros_like(case["q"])
    case["q"][0] = 7.0                                    # the lone atom: softmax over one score
    plan, splits = _plan(case)
    got = _attend(case, plan, splits, _device(case)).cpu().numpy()
    ns = case["node_splits"]
    assert np.array_equal(got[0], case["v"][0])
    for g in (1, 3):
        want = case["v"][ns[g]:ns[g + 1]].astype(np.float64).mean(axis=0)
        assert np.max(np.abs(got[ns[g]:ns[g + 1]] - want[None, :])) <= 2e-6


def test_packed_input_through_leading_dimensions():
    case, r32, r64 = _kernel_case("mixed-c064")
    plan, splits = _plan(case)
    dev = _device(case)
    c = case["heads"] * case["units"]
    packed = torch.cat([dev["q"], dev["k"], dev["v"]], dim=1).contiguous()          # (N, 3C)
    views = packed[:, :c], packed[:, c:2 * c], packed[:, 2 * c:]
    assert not views[1].is_contiguous() and views[1].stride(0) == 3 * c
    got = _attend(case, plan, splits, dev, *views)
    torch.cuda.synchronize()
    assert torch.equal(got, _attend(case, plan, splits, dev))


@pytest.mark.parametrize("e", [32, _ffi.MP_MAT_EPILOGUE_MAX_WIDTH])
@pytest.mark.parametrize("merge", ["concat", "sum"])
def test_merge_epilogue(merge, e):
    case, _, _ = _kernel_case("mixed-c064")
    plan, splits = _plan(case)
    dev = _device(case)
    heads, units = case["heads"], case["units"]
    rng = np.random.default_rng(23)
    n = int(case["node_splits"][-1])
    wm = mref.glorot(rng, units if merge == "sum" else heads * units, e)
    h = rng.normal(size=(n, e)).astype(np.float32)
    want = [mref.merged(mref.kernel_restate(case, dt), heads, units, torch.tensor(wm, dtype=dt), merge == "sum",
                        torch.tensor(h, dtype=dt)).numpy() for dt in (torch.float32, torch.float64)]
    code = _ffi.MP_MAT_MERGE_SUM if merge == "sum" else _ffi.MP_MAT_MERGE_CONCAT
    got = _attend(case, plan, splits, dev, wm=_cuda(wm), e=e, merge=code, h=_cuda(h))
    bare = _attend(case, plan, splits, dev, wm=_cuda(wm), e=e, merge=code)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (n, e) and bool(torch.isfinite(got).all())
    assert_rows_close(got.cpu().numpy(), want[0], want[1], what="epilogue %s E=%d" % (merge, e))
    assert_rows_close((got - _cuda(h)).cpu().numpy(), bare.cpu().numpy(), what="without the residual", rtol=1e-5)


def test_plain_build_ignores_the_epilogue_arguments():
    case, _, _ = _kernel_case("mixed-c064")
    plan, splits = _plan(case)
    dev = _device(case)
    plain = _attend(case, plan, splits, dev)
    other = _attend(case, plan, splits, dev, wm=None, e=32, merge=_ffi.MP_MAT_MERGE_SUM)
    torch.cuda.synchronize()
    assert torch.equal(plain, other)
    with pytest.raises(ValueError, match="epilogue"):   # units = 6 is outside the epilogue's sizes: refused, not served
        odd, _, _ = _kernel_case("mixed-c006")
        p6, s6 = _plan(odd)
        _attend(odd, p6, s6, _device(odd), wm=torch.zeros(6, 32, device="cuda"), e=32)


def test_out_of_range_sender_is_clamped_and_flagged():
    """A sender id past the batch, written into the plan's shifted column behind its validation: the kernel reads the
    clamped row and raises MP_FLAG_OOB; every row is still written and finite."""
    case, _, _ = _kernel_case("mixed-c008")
    plan, splits = _plan(case)
    dev = _device(case)
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    clean = _attend(case, plan, splits, dev, flags=flags)
    assert int(flags.item()) == 0
    n = int(case["node_splits"][-1])
    plan.cols[1, 3] = n + 1000
    plan.cols[1, 5] = -7
    got = _attend(case, plan, splits, dev, flags=flags)
    torch.cuda.synchronize()
    assert int(flags.item()) & _ffi.MP_FLAG_OOB
    assert bool(torch.isfinite(got).all()) and not torch.equal(got, clean)


# ------------------------------------------------------------------------------------------------ the head layer
def test_attention_head_layer():
    from gcnn_keras_amd.layers.conv.mat_conv import MATAttentionHead
    b = mref.model_batch(5, seed=77)                      # 5 molecules and an empty one
    rng = np.random.default_rng(24)
    ns, es = b["node_splits"], b["edge_splits"]
    n = int(ns[-1])
    hn = rng.normal(size=(n, 12)).astype(np.float32)
    p = mref.head_params(rng, 12, 6)
    for trafo, eye in (("exp", False), ("softmax", True), (None, False)):
        head = MATAttentionHead(units=6, lambda_attention=0.35, lambda_distance=0.25, add_identity=eye, dropout=0.1)
        head.trafo = trafo
        x = [_rag(hn, ns), _rag(b["node_coordinates"], ns), _rag(b["edge_weights"], es), _rag(b["edge_indices"], es)]
        head.ensure_built([t.shape for t in x])
        head.set_weights(list(p.values()))
        with torch.no_grad():
            head(x)
            count = _ffi.launch_count()
            got = head(x)
            assert _ffi.launch_count() - count == 4       # three Dense and the attention
        want = [mref.head_loop(torch.tensor(hn, dtype=dt), torch.tensor(b["node_coordinates"], dtype=dt),
                               torch.tensor(b["edge_weights"][:, 0], dtype=dt), b["edge_indices"], ns, es,
                               mref.params_to(p, dt), 6, trafo, 0.35, 0.25, 1.0 - 0.35 - 0.25, eye).numpy()
                for dt in (torch.float32, torch.float64)]
        assert tuple(got.values.shape) == (n, 6)
        assert_rows_close(got.values.cpu().numpy(), want[0], want[1], what="head %s" % trafo)


# ------------------------------------------------------------------------------------------------ the model
@functools.lru_cache(maxsize=None)
def _model_case(name):
    cfg = dict(mref.model_cases()[name])
    b = mref.model_batch()
    if name == "node-output":
        cfg["max_atoms"] = int(np.diff(b["node_splits"]).max()) + 3
    p = mref.model_params(np.random.default_rng(59), cfg)
    rows = lambda a: a.reshape(-1, a.shape[-1])
    return cfg, b, p, rows(mref.model_forward(p, cfg, b, torch.float32).numpy()), \
        rows(mref.model_forward(p, cfg, b, torch.float64).numpy())


def _inputs(b):
    ns, es = b["node_splits"], b["edge_splits"]
    return [_rag(b["node_number"], ns), _rag(b["node_coordinates"], ns), _rag(b["edge_weights"], es),
            _rag(b["edge_indices"], es)]


def _build(name):
    from gcnn_keras_amd.literature import MAT
    cfg, b, p, r32, r64 = _model_case(name)
    model = MAT.make_model(**mref.model_kwargs(cfg))
    model.set_weights(list(p.values()))
    return model, _inputs(b), cfg, r32, r64


def _rows(t):
    return t.reshape(-1, t.shape[-1]).cpu().numpy()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "layers"])
@pytest.mark.parametrize("name", sorted(mref.model_cases()))
def test_model_on_both_routes(name, fused):
    model, x, cfg, r32, r64 = _build(name)
    served = name != "layers-only"
    assert model.fused_attention_blocks == [served] * cfg["depth"]
    model.use_fused_attention = fused
    with torch.no_grad():
        eager = model(x)
        assert model.last_route == "eager"
        replayed = model(x)
        again = model(x)
    if name == "node-output":
        # the padded output needs the largest molecule on the host: the cached splits serve the capture
        assert tuple(eager.shape) == (len(x[0].row_splits) - 1, cfg["max_atoms"], 4)
        assert float(eager[-1].abs().max()) == 0.0      # the graph without atoms
    assert model.last_route == "graph"
    assert torch.equal(replayed, again) and replayed.data_ptr() != again.data_ptr()
    assert_rows_close(_rows(eager), r32, r64, what="%s eager" % name)
    assert_rows_close(_rows(replayed), r32, r64, what="%s replayed" % name)


def test_replay_with_rebound_inputs_predict_and_switch():
    model, x, cfg, r32, r64 = _build("default")
    _, b, p, _, _ = _model_case("default")
    with torch.no_grad():
        model(x), model(x)
        assert model.last_route == "graph"
        # new coordinates written into the bound input: the replay reads them
        moved = dict(b, node_coordinates=(b["node_coordinates"] * np.float32(0.9)).astype(np.float32))
        x[1].values.copy_(torch.from_numpy(moved["node_coordinates"]).cuda())
        got = model(x)
        assert model.last_route == "graph"
        want = [mref.model_forward(p, cfg, moved, dt).numpy() for dt in (torch.float32, torch.float64)]
        assert_rows_close(_rows(got), want[0], want[1], what="replay on re-bound coordinates")
        x[1].values.copy_(torch.from_numpy(b["node_coordinates"]).cuda())
        # weights changed in place: the packed q|k|v image is re-filled before the replay
        model.set_weights([np.float32(0.5) * w for w in model.get_weights()])
        halved = model(x)
        assert model.last_route == "graph"
        model.auto_graph = False
        assert_rows_close(_rows(halved), _rows(model(x)), what="replay after set_weights")
        model.auto_graph = True
        model.set_weights(list(p.values()))
        whole = model.predict(x)
        batched = model.predict(x, batch_size=5)
        assert tuple(whole.shape) == tuple(batched.shape)
        assert_rows_close(_rows(batched), r32, r64, what="predict in batches of 5")
        # the switch drops the captured graphs and flips the route; the two routes agree within the bar
        model.use_fused_attention = False
        layers = model(x)
        assert model.last_route == "eager" and model.use_fused_attention is False
        assert_rows_close(_rows(model.predict(x, batch_size=5)), r32, r64, what="predict in batches of 5, layers")
        model.use_fused_attention = True
        fused = model(x)
        assert model.last_route == "eager"
        assert_rows_close(_rows(layers), r32, r64, what="layer sequence")
        assert_rows_close(_rows(fused), _rows(layers), what="fused against the layer sequence")
        # a head switched behind the model's back keys the graphs and sends its block to the layer sequence
        model.attention_heads[0].use_fused_attention = False
        mixed = model(x)
        assert model.last_route == "eager" and model.use_fused_attention is False
        assert_rows_close(_rows(mixed), r32, r64, what="one block on the layers")


@pytest.mark.parametrize("merge", ["concat", "sum"])
def test_launch_counts_of_an_attention_sub_block(merge):
    from gcnn_keras_amd.literature import MAT
    cfg = mref.config(depth=1, merge_heads=merge)
    model = MAT.make_model(**mref.model_kwargs(cfg))
    b = mref.model_batch(6, seed=78)
    x = _inputs(b)
    ln1, block, heads = model.layers[4], model.attention_blocks[0], model.attention_heads
    rng = np.random.default_rng(25)
    h = _rag(rng.normal(size=(int(b["node_splits"][-1]), 32)).astype(np.float32), b["node_splits"])
    w = _rag(b["edge_weights"], b["edge_splits"])

    def fused_block():
        hn = ln1(h)
        assert block.route(hn, h)
        return block(hn, h, x[1], w, x[3])

    def layer_block():
        from gcnn_keras_amd.layers.modules import LazyAdd, LazyConcatenate
        hn = ln1(h)
        hs = [head([hn, x[1], w, x[3]]) for head in heads]
        hu = block.merge_dense((LazyAdd() if merge == "sum" else LazyConcatenate(axis=-1))(hs))
        return LazyAdd()([h, hu])

    with torch.no_grad():
        counts = []
        for fn in (fused_block, layer_block):
            fn()                                           # plans, CSR and the packed image are built once
            before = _ffi.launch_count()
            out = fn()
            counts.append(_ffi.launch_count() - before)
        both = fused_block(), layer_block()
        whole = []
        for flag in (True, False):
            model.use_fused_attention = flag
            model.auto_graph = False
            model(x)
            before = _ffi.launch_count()
            model(x)
            whole.append(_ffi.launch_count() - before)
    print("[mat] attention sub-block (%s): fused %d launches, layer sequence %d; one-block model %d / %d per forward"
          % (merge, counts[0], counts[1], whole[0], whole[1]))
    assert counts[0] <= 3
    assert counts[1] >= 1 + 4 * len(heads) + 3
    assert whole[1] - whole[0] == counts[1] - counts[0]
    assert_rows_close(both[0].values.cpu().numpy(), both[1].values.cpu().numpy(), what="block: fused against layers")
    assert tuple(out.values.shape) == (int(b["node_splits"][-1]), 32)


def test_grad_mode_is_refused_on_both_routes():
    model, x, cfg, _, _ = _build("sum")
    for fused in (True, False):
        model.use_fused_attention = fused
        model.requires_grad_(True)
        try:
            with torch.enable_grad(), pytest.raises(NotImplementedError, match="MAT"):
                model(x)
        finally:
            model.requires_grad_(False)
