"""CMPNN on the engine (csrc/mp_cmpnn.hip, csrc/mp_recurrent.hip, literature/CMPNN.py): the booster against the four-layer
sequence (equal bits), the directed edge update and the ragged GRU readout against the torch restatement
(tests/cmpnn_reference.py: float32 with the float64 twin as budget) and against the layers they replace, at the edges of the
kernels' tiles; the model on both routes, replayed and through ``predict``; the guards around a tape."""
import numpy as np
import pytest
import torch

import cmpnn_reference as ref
from gcnn_keras_amd import _ffi, synth
from gcnn_keras_amd.layers.conv.cmpnn_conv import (EDGE_TILE, CMPNNBoost, CMPNNCommunicate, boost_values,
                                                   directed_edge_update_values)
from gcnn_keras_amd.layers.conv.mpnn_conv import GRUUpdate
from gcnn_keras_amd.layers.pool.gru import PoolingNodesGRU
from gcnn_keras_amd.literature import CMPNN
from gcnn_keras_amd.ragged import RaggedTensor
from parity import assert_rows_close

pytestmark = pytest.mark.gpu

T = EDGE_TILE


def _rag(values, splits):
    return RaggedTensor.from_numpy(np.ascontiguousarray(values), np.asarray(splits, np.int64))


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype)


def _glorot(rng, shape, scale=1.0):
    limit = np.sqrt(6.0 / (shape[0] + shape[-1]))
    return (scale * rng.uniform(-limit, limit, size=shape)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------- booster
FOLD_DEGREES = [0, 1, 8, 9, 16, 17, 40]      # across the fold widths (8 and 16 rows) of the segment walk


def boost_graph(kind):
    """``(edge_indices (M, 2), node_splits, edge_splits)``: ``fold`` - one graph whose receivers 0..6 have FOLD_DEGREES
    incoming edges; ``tail_empty`` - the same followed by a graph of three nodes without edges; ``shuffled`` - two graphs
    with their edge lists in random order."""
    rng = np.random.default_rng(5)
    n = len(FOLD_DEGREES) + 2
    recv = np.repeat(np.arange(len(FOLD_DEGREES)), FOLD_DEGREES)
    idx = np.stack([recv, rng.integers(0, n, size=len(recv))], axis=1).astype(np.int64)
    if kind == "fold":
        return idx, [0, n], [0, len(idx)]
    if kind == "tail_empty":
        return idx, [0, n, n + 3], [0, len(idx), len(idx)]
    assert kind == "shuffled"
    second = np.stack([rng.integers(0, 5, size=23), rng.integers(0, 5, size=23)], axis=1).astype(np.int64)
    return (np.concatenate([idx[rng.permutation(len(idx))], second], axis=0), [0, n, n + 5],
            [0, len(idx), len(idx) + 23])


@pytest.mark.parametrize("width", [4, 64, 300])
@pytest.mark.parametrize("kind", ["fold", "tail_empty", "shuffled"])
def test_booster_has_the_bits_of_the_four_layers(kind, width):
    idx, ns, es = boost_graph(kind)
    rng = np.random.default_rng(width)
    h = _rag(rng.normal(size=(ns[-1], width)).astype(np.float32), ns)
    he = _rag(rng.normal(size=(es[-1], width)).astype(np.float32), es)
    edi = _rag(idx, es)
    recv = ref.flat_indices({"edge_indices": idx, "edge_indices_reverse": np.zeros(len(idx)), "node_splits": ns,
                             "edge_splits": es})[0]
    for method in ("sum", "mean"):
        for m_only in (False, True):
            lay = CMPNNBoost(pooling_method=method, m_only=m_only)
            with torch.no_grad():
                fused = lay([h, he, edi])
                lay.use_fused_communicate = False
                launches = _ffi.launch_count()
                seq = lay([h, he, edi])
                assert _ffi.launch_count() - launches == (3 if m_only else 4)
            assert lay.fused_communicate is True
            what = "booster %s F=%d %s m_only=%s" % (kind, width, method, m_only)
            assert torch.equal(fused.values, seq.values), what
            r32, r64 = (ref.booster(_t(h.values.cpu(), dt), _t(he.values.cpu(), dt), recv, method, m_only).numpy()
                        for dt in (torch.float32, torch.float64))
            assert_rows_close(fused.values.cpu().numpy(), r32, r64, what=what)
            if not m_only:      # receivers without edges keep h exactly
                lone = np.bincount(recv.numpy(), minlength=ns[-1]) == 0
                assert lone.any() and torch.equal(fused.values[torch.from_numpy(lone).cuda()],
                                                  h.values[torch.from_numpy(lone).cuda()])


def test_booster_refuses_what_it_does_not_serve():
    idx, ns, es = boost_graph("fold")
    h, he, edi = _rag(np.zeros((ns[-1], 6), np.float32), ns), _rag(np.zeros((es[-1], 6), np.float32), es), _rag(idx, es)
    with pytest.raises(ValueError):
        boost_values(h, he, edi, _ffi.MP_SUM)                    # width 6 is no multiple of 4
    lay = CMPNNBoost(pooling_method="sum")
    with torch.no_grad():
        out = lay([h, he, edi])                                  # ... and takes the layer sequence
    assert lay.fused_communicate is False and tuple(out.values.shape) == (ns[-1], 6)


# ------------------------------------------------------------------------------------------------------- edge update
def edge_case(edges, width, reverse="mix", seed=0):
    """Two graphs (one for fewer than two edges) that share ``edges`` directed edges over 70 + 45 nodes (more node rows
    than an edge tile has edges), random senders, reverse positions drawn over the whole graph's list (so they point into
    other tiles): ``mix`` - a third without a reverse (-1), ``none`` - all -1, ``self`` - every edge its own reverse."""
    rng = np.random.default_rng(seed + 7 * edges + width)
    sizes = [70, 45] if edges >= 2 else [70]
    counts = [edges - edges // 3, edges // 3] if edges >= 2 else [edges]
    idx, pair = [], []
    for n, m in zip(sizes, counts):
        idx.append(np.stack([np.sort(rng.integers(0, n, size=m)), rng.integers(0, n, size=m)], axis=1))
        if reverse == "none":
            pair.append(np.full(m, -1))
        elif reverse == "self":
            pair.append(np.arange(m))
        else:
            pair.append(np.where(rng.random(m) < 1 / 3, -1, rng.integers(0, max(m, 1), size=m)))
    ns, es = np.concatenate([[0], np.cumsum(sizes)]), np.concatenate([[0], np.cumsum(counts)])
    b = {"edge_indices": np.concatenate(idx).astype(np.int64).reshape(-1, 2),
         "edge_indices_reverse": np.concatenate(pair).astype(np.int64).reshape(-1, 1), "node_splits": ns, "edge_splits": es}
    b["h"] = (0.5 * rng.normal(size=(ns[-1], width))).astype(np.float32)
    b["he"] = (0.5 * rng.normal(size=(edges, width))).astype(np.float32)
    b["he0"] = (0.5 * rng.normal(size=(edges, width))).astype(np.float32)
    return b


def make_round(width, seed, use_bias=True, activation="linear", edge_activation="relu", method="sum"):
    rng = np.random.default_rng(seed)
    lay = CMPNNCommunicate(edge_dense={"units": width, "activation": activation, "use_bias": use_bias},
                           edge_activation={"activation": edge_activation}, pooling_kwargs={"pooling_method": method},
                           dropout={"rate": 0.1})
    lay.ensure_built([(None, None, width)] * 3 + [(None, None, 2), (None, None, 1)])
    bias = [rng.uniform(-0.1, 0.1, width).astype(np.float32)] if use_bias else []
    lay.set_weights([_glorot(rng, (width, width))] + bias)
    return lay


def edge_sequence(lay, h, he, he0, edi, pairs):
    """The reference's layers of the edge update, on the round's own layers."""
    x = lay.lay_subtract([lay.lay_gather_out([h, edi]), lay.lay_gather_pairs([he, pairs])])
    return lay.lay_act(lay.lay_add([lay.lay_dense(x), he0]))


def check_edge_update(edges, width, reverse="mix", **config):
    b = edge_case(edges, width, reverse)
    lay = make_round(width, seed=edges + width, **config)
    assert lay.fused_communicate is True
    ns, es = b["node_splits"], b["edge_splits"]
    h, he, he0 = _rag(b["h"], ns), _rag(b["he"], es), _rag(b["he0"], es)
    edi, pairs = _rag(b["edge_indices"], es), _rag(b["edge_indices_reverse"], es)
    dense = lay.lay_dense
    args = (h, he, he0, edi, pairs, dense.kernel, dense.bias, dense.activation, lay.lay_act.activation)
    with torch.no_grad():
        fused = directed_edge_update_values(*args).values
        again = directed_edge_update_values(*args).values
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            other = directed_edge_update_values(*args).values
        side.synchronize()
        seq = edge_sequence(lay, h, he, he0, edi, pairs).values
    assert tuple(fused.shape) == (edges, width) == tuple(seq.shape)
    assert torch.equal(fused, again) and torch.equal(fused, other)
    what = "edge update E=%d F=%d %s %s" % (edges, width, reverse, config)
    if edges == 0:           # parity.py takes no tensor without rows: an empty result is held to its shape
        return
    _, send, rev = ref.flat_indices(b)
    w = [_t(a, torch.float32) for a in lay.get_weights()]
    r32, r64 = (ref.edge_update(_t(b["h"], dt), _t(b["he"], dt), _t(b["he0"], dt), send, rev, w[0].to(dt),
                                w[1].to(dt) if dense.bias is not None else None, dense.activation,
                                lay.lay_act.activation).numpy() for dt in (torch.float32, torch.float64))
    assert_rows_close(fused.cpu().numpy(), r32, r64, what=what)
    assert_rows_close(fused.cpu().numpy(), seq.cpu().numpy(), what=what + " vs layer sequence")
    print("[cmpnn] %s: bits equal to the layer sequence: %s" % (what, bool(torch.equal(fused, seq))))


@pytest.mark.parametrize("width", [300, 64, 4])
@pytest.mark.parametrize("edges", [0, 1, T - 1, T, T + 1, 2 * T + 1])
def test_edge_update_at_tile_edges(edges, width):
    check_edge_update(edges, width)


@pytest.mark.parametrize("reverse,config", [
    ("none", dict(use_bias=False, activation="relu", edge_activation="swish")),
    ("self", dict(use_bias=True, activation="linear", edge_activation="linear")),
    ("mix", dict(use_bias=True, activation="relu", edge_activation="relu")),
    ("mix", dict(use_bias=False, activation="linear", edge_activation="swish")),
    ("none", dict(use_bias=True, activation="linear", edge_activation="relu")),
    ("self", dict(use_bias=False, activation="relu", edge_activation="linear")),
])
def test_edge_update_configurations(reverse, config):
    check_edge_update(2 * T + 1, 300, reverse, **config)
    check_edge_update(T + 1, 64, reverse, **config)


def test_edge_update_refuses_aliasing_out_with_he():
    b = edge_case(T + 1, 64)
    lay = make_round(64, seed=1)
    ns, es = b["node_splits"], b["edge_splits"]
    h, he, he0 = _rag(b["h"], ns), _rag(b["he"], es), _rag(b["he0"], es)
    edi, pairs = _rag(b["edge_indices"], es), _rag(b["edge_indices_reverse"], es)
    before = he.values.clone()
    with pytest.raises(ValueError, match="alias"):
        directed_edge_update_values(h, he, he0, edi, pairs, lay.lay_dense.kernel, lay.lay_dense.bias, "linear", "relu",
                                    out=he.values)
    assert torch.equal(he.values, before)
    spare = torch.empty_like(he.values)
    out = directed_edge_update_values(h, he, he0, edi, pairs, lay.lay_dense.kernel, lay.lay_dense.bias, "linear", "relu",
                                      out=spare)
    assert out.values.data_ptr() == spare.data_ptr()


@pytest.mark.parametrize("method", ["sum", "mean"])
def test_round_fused_against_layer_sequence_and_restatement(method):
    b = synth.cmpnn_batch(5, seed=9)
    width = 64
    rng = np.random.default_rng(2)
    ns, es = b["node_splits"], b["edge_splits"]
    hv = (0.3 * rng.normal(size=(ns[-1], width))).astype(np.float32)
    ev = (0.3 * rng.normal(size=(es[-1], width))).astype(np.float32)
    lay = make_round(width, seed=4, method=method)
    x = [_rag(hv, ns), _rag(ev, es), _rag(ev, es), _rag(b["edge_indices"], es), _rag(b["edge_indices_reverse"], es)]
    with torch.no_grad():
        lay(x)                                   # index plans and CSR are built once per batch, outside the count
        launches = _ffi.launch_count()
        h1, e1 = lay(x)
        fused_launches = _ffi.launch_count() - launches
        lay.use_fused_communicate = False
        lay(x)
        launches = _ffi.launch_count()
        h2, e2 = lay(x)
        seq_launches = _ffi.launch_count() - launches
    print("[cmpnn] launches per round: fused %d, layer sequence %d" % (fused_launches, seq_launches))
    assert fused_launches == 2 and seq_launches >= 11
    assert torch.equal(h1.values, h2.values)
    recv, send, rev = ref.flat_indices(b)
    w = lay.get_weights()
    r32, r64 = (ref.communicate_round(_t(hv, dt), _t(ev, dt), _t(ev, dt), recv, send, rev, _t(w[0], dt), _t(w[1], dt),
                                      "linear", "relu", method) for dt in (torch.float32, torch.float64))
    assert_rows_close(e1.values.cpu().numpy(), r32[1].numpy(), r64[1].numpy(), what="round he (%s)" % method)
    assert_rows_close(h1.values.cpu().numpy(), r32[0].numpy(), r64[0].numpy(), what="round h (%s)" % method)
    assert_rows_close(e1.values.cpu().numpy(), e2.values.cpu().numpy(), what="round he vs layer sequence (%s)" % method)


# --------------------------------------------------------------------------------------------------------------- GRU
def make_gru(units, in_dim, seed, use_bias=True, **kwargs):
    rng = np.random.default_rng(seed)
    lay = PoolingNodesGRU(units=units, use_bias=use_bias, **kwargs)
    lay.ensure_built((None, None, in_dim))
    ws = [_glorot(rng, (in_dim, 3 * units)), _glorot(rng, (units, 3 * units))]
    if use_bias:
        ws.append(rng.uniform(-0.1, 0.1, (2, 3 * units)).astype(np.float32))
    lay.set_weights(ws)
    return lay


def check_gru(lengths, units, in_dim, use_bias=True, seed=0):
    rng = np.random.default_rng(seed + units + in_dim + len(lengths))
    splits = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    xv = (0.5 * rng.normal(size=(int(splits[-1]), in_dim))).astype(np.float32)
    lay = make_gru(units, in_dim, seed + 1, use_bias)
    x = _rag(xv, splits)
    with torch.no_grad():
        got, again = lay(x), lay(x)
    assert tuple(got.shape) == (len(lengths), units)             # one row per graph, trailing empty graphs included
    assert torch.equal(got, again)
    empty = torch.from_numpy(np.asarray(lengths) == 0).cuda()
    assert torch.all(got[empty] == 0.0)                          # a graph without nodes returns the zero state
    w = lay.get_weights()
    r32, r64 = (ref.gru_ragged_last(_t(xv, dt), splits, _t(w[0], dt), _t(w[1], dt),
                                    _t(w[2], dt) if use_bias else None).numpy() for dt in (torch.float32, torch.float64))
    if np.any(r64 != 0.0):
        assert_rows_close(got.cpu().numpy(), r32, r64, what="GRU lengths %s u=%d in=%d bias=%s"
                          % (list(lengths)[:8], units, in_dim, use_bias))
    else:
        assert not torch.any(got != 0.0)
    return lay, x, got


@pytest.mark.parametrize("graphs", [1, 15, 16, 17, 33])
def test_gru_graph_counts(graphs):
    rng = np.random.default_rng(graphs)
    check_gru(rng.integers(0, 7, size=graphs), 64, 12)


@pytest.mark.parametrize("lengths", [[0] * 5, [1] * 17, [1, 40], [0, 3, 2], [3, 0, 2], [3, 2, 0]],
                         ids=["all0", "all1", "1_40", "zero_first", "zero_middle", "zero_last"])
def test_gru_lengths(lengths):
    check_gru(lengths, 8, 12)
    check_gru(lengths, 64, 12)


@pytest.mark.parametrize("units,in_dim", [(300, 300), (300, 12), (64, 300), (8, 12), (512, 12)])
def test_gru_widths(units, in_dim):
    check_gru([5, 0, 3, 1, 7, 2, 4, 6, 2, 3, 1, 0, 5, 4, 3, 2, 6], units, in_dim)


def test_gru_without_bias():
    check_gru([4, 0, 9, 1, 3, 2, 6, 5, 2], 64, 12, use_bias=False)
    check_gru([2, 5, 0, 1] * 5, 300, 12, use_bias=False)


def test_gru_single_graph_is_successive_gru_updates():
    length, units, in_dim = 6, 64, 12
    lay, x, got = check_gru([length], units, in_dim)
    cell = GRUUpdate(units=units)
    cell.ensure_built([(None, None, units), (None, None, in_dim)])
    cell.set_weights(lay.get_weights())
    one = np.array([0, 1], np.int64)
    state = _rag(np.zeros((1, units), np.float32), one)
    with torch.no_grad():
        for t in range(length):
            state = cell([state, _rag(x.values[t:t + 1].cpu().numpy(), one)])
    assert_rows_close(got.cpu().numpy(), state.values.cpu().numpy(), what="GRU vs %d GRUUpdate steps" % length)


def test_gru_refuses_a_tape():
    lay = make_gru(8, 12, 0)
    x = _rag(np.ones((3, 12), np.float32), [0, 3])
    x.values.requires_grad_(True)
    with pytest.raises(NotImplementedError):
        lay(x)
    with torch.no_grad():
        assert tuple(lay(x).shape) == (1, 8)


# ------------------------------------------------------------------------------------------------------------- model
BATCH_SEED, WEIGHT_SEED = ref.MODEL_SEED      # draws whose float32 restatement is within 5e-6 of float64 (test_cmpnn_api.py)


def model_inputs(b, features=False):
    ns, es = b["node_splits"], b["edge_splits"]
    nodes = _rag(b["node_attributes"], ns) if features else _rag(b["node_number"].astype(np.float32), ns)
    edges = _rag(b["edge_attributes"], es) if features else _rag(b["edge_number"].astype(np.float32), es)
    return [nodes, edges, _rag(b["edge_indices"], es), _rag(b["edge_indices_reverse"], es)]


def make_model(width, gru=True, features=False, weight_seed=WEIGHT_SEED, **extra):
    m = CMPNN.make_model(**ref.model_kwargs(width, gru, features, **extra))
    m.set_weights(ref.parity_weights(m, weight_seed))
    return m


def restate(m, b, gru=True, features=False, output_embedding="graph", depth=5):
    return [ref.forward(m.get_weights(), b, dt, depth=depth, embed_nodes=not features, embed_edges=not features,
                        use_final_gru=gru, output_embedding=output_embedding)["out"].numpy()
            for dt in (torch.float32, torch.float64)]


@pytest.mark.parametrize("width,gru,features", ref.MODEL_CASES)
def test_model_routes_against_the_restatement(width, gru, features):
    b = synth.cmpnn_batch(12, seed=BATCH_SEED)
    m = make_model(width, gru, features)
    assert m.fused_communicate_rounds == [True] * 4
    x = model_inputs(b, features)
    r32, r64 = restate(m, b, gru, features)
    what = "CMPNN F=%d %s %s" % (width, "gru" if gru else "pool", "features" if features else "embedding")
    with torch.no_grad():
        m.auto_graph = False
        launches = _ffi.launch_count()
        fused = m(x)
        fused_launches = _ffi.launch_count() - launches
        m.use_fused_communicate = False
        launches = _ffi.launch_count()
        seq = m(x)
        seq_launches = _ffi.launch_count() - launches
    assert tuple(fused.shape) == (12, 1)
    print("[cmpnn] %s: engine calls fused %d, layer sequence %d" % (what, fused_launches, seq_launches))
    assert fused_launches < seq_launches
    assert_rows_close(fused.cpu().numpy(), r32, r64, what=what + ", fused")
    assert_rows_close(seq.cpu().numpy(), r32, r64, what=what + ", layer sequence")


def test_model_node_embedding():
    b = synth.cmpnn_batch(12, seed=ref.NODE_SEED[0])
    m = make_model(64, weight_seed=ref.NODE_SEED[1], output_embedding="node")
    x = model_inputs(b)
    r32, r64 = restate(m, b, output_embedding="node")
    with torch.no_grad():
        out = m(x)
    rows = out.values if isinstance(out, RaggedTensor) else out
    # output_to_tensor pads every graph to the longest: compare graph by graph
    ns = b["node_splits"]
    assert tuple(rows.shape) == (12, int(np.max(np.diff(ns))), 1)
    got = np.concatenate([rows[g, :ns[g + 1] - ns[g]].cpu().numpy() for g in range(12)])
    assert_rows_close(got, r32, r64, what="CMPNN node embedding")


def test_model_eager_replayed_predict_and_switch():
    b = synth.cmpnn_batch(12, seed=BATCH_SEED)
    m = make_model(300)
    x = model_inputs(b)
    r32, r64 = restate(m, b)
    with torch.no_grad():
        eager = m(x)
        assert m.last_route == "eager"
        second, third = m(x), m(x)
        assert m.last_route == "graph"
        served = m.predict(x, batch_size=5)
        m.use_fused_communicate = False
        assert all(not lay.use_fused_communicate for lay in m.communicate_layers)
        seq = m(x)
        assert m.last_route == "eager"                       # flipping the switch dropped the captured graphs
        m(x)
        seq_replayed = m(x)
        assert m.last_route == "graph"
        m.use_fused_communicate = True
        back = m(x)
        assert m.last_route == "eager"
    assert torch.equal(eager, second) and torch.equal(eager, third) and torch.equal(eager, back)
    assert torch.equal(seq, seq_replayed)
    assert tuple(served.shape) == (12, 1)
    assert_rows_close(eager.cpu().numpy(), r32, r64, what="CMPNN default widths, fused")
    assert_rows_close(served.cpu().numpy(), r32, r64, what="CMPNN default widths, predict(batch_size=5)")
    assert_rows_close(served.cpu().numpy(), eager.cpu().numpy(), what="predict vs one call")
    assert_rows_close(seq.cpu().numpy(), r32, r64, what="CMPNN default widths, layer sequence")


def test_model_unserved_width_takes_the_layer_sequence():
    b = synth.cmpnn_batch(12, seed=BATCH_SEED)
    m = make_model(302, depth=3)
    assert m.fused_communicate_rounds == [False, False]
    x = model_inputs(b)
    r32, r64 = restate(m, b, depth=3)
    with torch.no_grad():
        out = m(x)
    assert_rows_close(out.cpu().numpy(), r32, r64, what="CMPNN width 302 (layer sequence)")


# ------------------------------------------------------------------------------------------------------------ guards
def test_guards_around_a_tape():
    b = synth.cmpnn_batch(4, seed=BATCH_SEED)
    m = make_model(64, depth=3)
    x = model_inputs(b)
    before = [w.copy() for w in m.get_weights()]
    with torch.no_grad():
        first = m(x)
    m.requires_grad_(True)
    with pytest.raises(NotImplementedError):
        m(x)                                                 # max pooling has no reverse rule: never a silent zero gradient
    with torch.no_grad():
        assert torch.equal(m(x), first)                      # under no_grad the model runs
    m.requires_grad_(False)
    assert torch.equal(m(x), first)                          # ... and again after requires_grad_(False)
    assert all(np.array_equal(a, w) for a, w in zip(before, m.get_weights()))
    assert all(t.grad is None for t in m.trainable_weights)


def test_round_with_an_input_on_a_tape_takes_the_layer_sequence():
    b = edge_case(T + 1, 64)
    lay = make_round(64, seed=3)
    ns, es = b["node_splits"], b["edge_splits"]
    x = [_rag(b["h"], ns), _rag(b["he"], es), _rag(b["he0"], es), _rag(b["edge_indices"], es),
         _rag(b["edge_indices_reverse"], es)]
    with torch.no_grad():
        h_ref, he_ref = lay(x)
    x[2].values.requires_grad_(True)          # he0 enters behind the pooling: the layers carry its gradient
    launches = _ffi.launch_count()
    h, he = lay(x)
    assert _ffi.launch_count() - launches >= 11
    assert he.values.requires_grad and not h.values.requires_grad
    he.values.sum().backward()
    assert x[2].values.grad is not None and float(x[2].values.grad.abs().sum()) > 0.0
    assert torch.equal(h.values, h_ref.values)
    assert_rows_close(he.values.detach().cpu().numpy(), he_ref.values.cpu().numpy(), what="round on a tape vs fused")
    x[1].values.requires_grad_(True)          # he feeds the max pooling: refused, not a zero gradient
    with pytest.raises(NotImplementedError):
        lay(x)
