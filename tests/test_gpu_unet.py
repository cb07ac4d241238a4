"""Graph U-Net on csrc/mp_topk.hip: ``PoolingTopK`` (selection and induced edges), ``AdjacencyPower``, ``UnPoolingTopK``
and the model with its gradients, all against tests/unet_reference.py (float32 and float64).

Index outputs (maps, re-indexed edges, row splits, the ``A^n`` index lists) are compared exactly, float outputs with
``parity.assert_rows_close`` at its defaults.  Exact comparisons are made only where the reference alone is
unambiguous: scores that are exact in float32 (integer features, ``p`` = ones, ``F`` in {4, 16}: ``1 / ||p||`` is a power
of two), integer adjacency weights, or random inputs whose margins the test asserts first (tests/test_unet_api.py states
the conditions)."""
import functools

import numpy as np
import pytest
import torch

import unet_reference as uref
from gcnn_keras_amd import _ffi, synth
from parity import assert_rows_close
from test_unet_api import FEATURE_INPUTS

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 5, 15, 63, 64, 65, 300, 0]   # the last graph is empty: trailing empty rows everywhere


def _rag(values, splits):
    from gcnn_keras_amd.ragged import RaggedTensor
    return RaggedTensor.from_numpy(np.ascontiguousarray(values), np.asarray(splits, dtype=np.int64))


def _splits(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def _ring_edges(rng, sizes, extra=2, shuffle=True, loops=False):
    """Per graph a directed ring both ways plus ``extra`` random pairs per node (no duplicates), optionally self loops,
    optionally shuffled (an unsorted list)."""
    idx = []
    for n in sizes:
        pairs = set()
        for a in range(n):
            if n > 1:
                pairs.add((a, (a + 1) % n))
                pairs.add(((a + 1) % n, a))
            for _ in range(extra if n > 2 else 0):
                b = int(rng.integers(0, n))
                if b != a:
                    pairs.add((a, b))
            if loops and a % 3 == 0:
                pairs.add((a, a))
        e = np.array(sorted(pairs), dtype=np.int64).reshape(-1, 2)
        if shuffle and len(e):
            e = e[rng.permutation(len(e))]
        idx.append(e)
    return idx


def _pool_reference(x, p, edges, idx_list, ns, es, k, dtype):
    """PoolingTopK per graph -> concatenated outputs and splits (sample indexing)."""
    out = {"x": [], "e": [], "idx": [], "map_n": [], "map_e": [], "nl": [], "el": []}
    pt = torch.from_numpy(p).to(dtype)
    for g in range(len(ns) - 1):
        xg = torch.from_numpy(x[ns[g]:ns[g + 1]]).to(dtype)
        eg = torch.from_numpy(edges[es[g]:es[g + 1]]).to(dtype)
        x_new, e_new, idx_new, map_n, map_e, _ = uref.pooling_topk(xg, eg, idx_list[g], pt, k)
        for key, v in (("x", x_new.numpy()), ("e", e_new.numpy()), ("idx", idx_new), ("map_n", map_n), ("map_e", map_e)):
            out[key].append(v)
        out["nl"].append(len(map_n))
        out["el"].append(len(map_e))
    cat = {key: np.concatenate(out[key], axis=0) for key in ("x", "e", "idx", "map_n", "map_e")}
    cat["ns"], cat["es"] = _splits(out["nl"]), _splits(out["el"])
    return cat


def _host(r):
    return r.values.detach().cpu().numpy(), r.row_splits.cpu().numpy()


def _check_pooled(got, maps, want, want64=None, batch_offsets=None, what=""):
    """``got`` / ``maps``: the layer's outputs; ``want``: ``_pool_reference`` in float32 (``want64`` in float64).
    ``batch_offsets``: ``(old node splits, old edge splits)`` when the layer ran with node_indexing "batch"."""
    (xv, xs), (ev, esp), (iv, isp) = (_host(t) for t in got)
    (mn, mns), (me, mes) = (_host(t) for t in maps)
    for s in (xs, mns):
        assert np.array_equal(s, want["ns"]), what
    for s in (esp, isp, mes):
        assert np.array_equal(s, want["es"]), what
    w_idx, w_mn, w_me = want["idx"].copy(), want["map_n"].copy(), want["map_e"].copy()
    if batch_offsets is not None:
        ns_old, es_old = batch_offsets
        g_of_node = np.repeat(np.arange(len(want["ns"]) - 1), np.diff(want["ns"]))
        g_of_edge = np.repeat(np.arange(len(want["es"]) - 1), np.diff(want["es"]))
        w_mn += ns_old[g_of_node]
        w_me += es_old[g_of_edge]
        w_idx += want["ns"][g_of_edge][:, None]
    assert np.array_equal(mn, w_mn), what + ": map_nodes"
    assert np.array_equal(me, w_me), what + ": map_edges"
    assert np.array_equal(iv, w_idx.reshape(-1, 2)), what + ": edge_indices"
    assert xv.shape == want["x"].shape and ev.shape == want["e"].shape, what
    if len(xv):
        assert_rows_close(xv, want["x"], None if want64 is None else want64["x"], what=what + " nodes")
    assert np.array_equal(ev, want["e"]), what + ": the edge rows are copies"
    # the attached plan is the plan a fresh preparation gives
    if batch_offsets is None and len(iv):
        plan = got[2].index_plan(got[0])
        fresh = _rag(iv, isp).index_plan(_rag(xv, xs))
        assert torch.equal(plan.cols[:, :plan.M], fresh.cols[:, :fresh.M])
        assert torch.equal(plan.csr(0)[0], fresh.csr(0)[0])


# ------------------------------------------------------------------------------------------------ selection
def _exact_features(mode, n, f, rng):
    if mode == "all_equal":
        return np.full((n, f), 2.0, dtype=np.float32)
    if mode == "two_level":          # scores in two groups per graph: every cut but k = 1.0 falls inside a tie group
        x = np.zeros((n, f), dtype=np.float32)
        x[rng.random(n) < 0.33, 0] = 4.0   # about two thirds score 0: the cuts at 0.1, 0.3 and 0.5 fall among them
        return x
    return rng.integers(-3, 4, size=(n, f)).astype(np.float32)


@pytest.mark.parametrize("mode", ["random", "all_equal", "two_level"])
@pytest.mark.parametrize("f", [4, 16])
@pytest.mark.parametrize("k", [0.1, 0.3, 0.5, 1.0])
def test_selection_with_exact_scores(k, f, mode):
    from gcnn_keras_amd.layers.pool.topk import PoolingTopK
    rng = np.random.default_rng(100 + f)
    ns = _splits(SIZES)
    x = _exact_features(mode, int(ns[-1]), f, rng)
    idx_list = _ring_edges(rng, SIZES)
    es = _splits([len(e) for e in idx_list])
    edges = rng.normal(size=(int(es[-1]), 3)).astype(np.float32)
    p = np.ones((1, f), dtype=np.float32)
    layer = PoolingTopK(k=k, kernel_initializer="ones")
    inputs = [_rag(x, ns), _rag(edges, es), _rag(np.concatenate(idx_list), es)]
    with torch.no_grad():
        got, maps = layer(inputs)
        again, _ = layer(inputs)
    w32, w64 = (_pool_reference(x, p, edges, idx_list, ns, es, k, dt) for dt in (torch.float32, torch.float64))
    assert np.array_equal(w32["map_n"], w64["map_n"])           # exact scores: one answer in either precision
    _check_pooled(got, maps, w32, w64, what="k=%g F=%d %s" % (k, f, mode))
    rem, keep = zip(*(uref.topk_counts(k, n) for n in SIZES))
    assert np.array_equal(np.diff(_host(got[0])[1]), keep)
    if k == 0.3:
        assert (rem[3], rem[4]) == (2, 4)                       # 5 nodes lose 2, 15 lose 4
    for a, b in zip(got, again):
        assert torch.equal(a.values, b.values)                  # equal bits on every call
    if mode != "random" and k < 1.0:
        # ties across the cut: the kept ids of a tie group are its largest ones
        s = x.sum(axis=1)
        lo, hi = int(ns[8]), int(ns[9])
        kept = np.sort(_host(maps[0])[0][w32["ns"][8]:w32["ns"][9]])
        cut = s[lo:hi][kept].min()
        tied = np.nonzero(s[lo:hi] == cut)[0]
        assert len(tied) > np.sum(s[lo:hi][kept] == cut) > 0
        assert np.array_equal(kept[s[lo:hi][kept] == cut], tied[-int(np.sum(s[lo:hi][kept] == cut)):])


def test_selection_random_features_f32():
    """F = 32, normal features and a random ``p``: scores are inexact, so the comparison is the float one, valid while
    every gap between adjacent sorted scores of a graph is at least 1e-4 of the largest score (asserted)."""
    from gcnn_keras_amd.layers.pool.topk import PoolingTopK
    rng = np.random.default_rng(23)
    ns = _splits(SIZES)
    p = rng.uniform(0.5, 1.5, size=(1, 32)).astype(np.float32)
    x = _separated_features(rng, SIZES, p)
    for g in range(len(SIZES)):
        s = uref.scores(torch.from_numpy(x[ns[g]:ns[g + 1]]).double(), torch.from_numpy(p).double()).numpy()
        if len(s) > 1:
            assert np.diff(np.sort(s)).min() >= 1e-4 * np.abs(s).max(), "the committed seed must keep the scores apart"
    idx_list = _ring_edges(rng, SIZES)
    es = _splits([len(e) for e in idx_list])
    edges = rng.normal(size=(int(es[-1]), 1)).astype(np.float32)
    layer = PoolingTopK(k=0.3)
    layer.ensure_built([(None, None, 32), (None, None, 1), (None, None, 2)])
    layer.set_weights([p])
    with torch.no_grad():
        got, maps = layer([_rag(x, ns), _rag(edges, es), _rag(np.concatenate(idx_list), es)])
    w32, w64 = (_pool_reference(x, p, edges, idx_list, ns, es, 0.3, dt) for dt in (torch.float32, torch.float64))
    xv, xs = _host(got[0])
    assert np.array_equal(xs, w32["ns"])
    assert_rows_close(xv, w32["x"], w64["x"], what="F=32 random features")


def _separated_features(rng, sizes, p, apart=1e-3):
    """Normal feature rows, drawn again while the row's score is within ``apart`` of another score of its graph: the
    random features conditioned on the gap condition (scores are N(0, 1), so 1e-3 is at least 1e-4 of the largest)."""
    unit = (p / np.sqrt((p.astype(np.float64) ** 2).sum())).astype(np.float64)[0]
    rows = []
    for n in sizes:
        seen = []
        while len(seen) < n:
            row = rng.normal(size=p.shape[1]).astype(np.float32)
            s = float(row.astype(np.float64) @ unit)
            if all(abs(s - t) >= apart for t in seen):
                seen.append(s)
                rows.append(row)
    return np.array(rows, dtype=np.float32).reshape(-1, p.shape[1])


# ------------------------------------------------------------------------------------------------ induced edges
def _edge_case_batch():
    """Integer features, p = ones, k = 0.5.  Graph 0 (6 nodes): node 5 is kept and receives only from removed nodes.
    Graph 1 (4 nodes): every edge touches a removed node.  Graph 2 (5 nodes): self loops on kept and removed nodes.
    Graph 3: no nodes.  Graph 4 (3 nodes, no edges).  All lists unsorted."""
    scores = [[0, 1, 2, 7, 8, 9], [5, 0, 6, 1], [3, 0, 4, 1, 5], [], [1, 2, 3]]
    idx = [np.array([[5, 0], [5, 1], [3, 4], [4, 3], [0, 5], [3, 5], [4, 4], [1, 2], [5, 2], [3, 0]]),
           np.array([[0, 1], [1, 0], [2, 3], [3, 2], [1, 3], [0, 3]]),
           np.array([[4, 4], [1, 1], [0, 2], [2, 0], [0, 0], [3, 4], [4, 2], [2, 4], [4, 0]]),
           np.zeros((0, 2)), np.zeros((0, 2))]
    idx = [np.asarray(e, dtype=np.int64) for e in idx]
    sizes = [len(s) for s in scores]
    x = np.zeros((sum(sizes), 4), dtype=np.float32)
    x[:, 0] = np.concatenate([np.asarray(s, dtype=np.float32) for s in scores])
    ns, es = _splits(sizes), _splits([len(e) for e in idx])
    edges = np.arange(int(es[-1]) * 2, dtype=np.float32).reshape(-1, 2)
    return x, idx, ns, es, edges


@pytest.mark.parametrize("node_indexing", ["sample", "batch"])
def test_induced_edges_on_hand_made_graphs(node_indexing):
    from gcnn_keras_amd.layers.pool.topk import PoolingTopK
    x, idx_list, ns, es, edges = _edge_case_batch()
    p = np.ones((1, 4), dtype=np.float32)
    w32 = _pool_reference(x, p, edges, idx_list, ns, es, 0.5, torch.float32)
    # the situations this test is about do occur
    assert w32["map_n"][:3].tolist() == [3, 4, 5] and not np.any(w32["idx"][:int(w32["es"][1])][:, 0] == 2), \
        "graph 0: node 5 (new id 2) keeps no sender"
    assert w32["es"][2] == w32["es"][1] and es[2] > es[1], "graph 1 loses all its edges"
    loops = w32["idx"][int(w32["es"][2]):int(w32["es"][3])]
    assert np.sum(loops[:, 0] == loops[:, 1]) == 2, "graph 2 keeps the self loops of kept nodes"
    flat = np.concatenate(idx_list).astype(np.int64)
    if node_indexing == "batch":
        flat = flat + np.repeat(ns[:-1], np.diff(es))[:, None]
    layer = PoolingTopK(k=0.5, kernel_initializer="ones", node_indexing=node_indexing)
    with torch.no_grad():
        got, maps = layer([_rag(x, ns), _rag(edges, es), _rag(flat, es)])
    _check_pooled(got, maps, w32, batch_offsets=(ns, es) if node_indexing == "batch" else None, what=node_indexing)


# ------------------------------------------------------------------------------------------------ adjacency power
def _power_reference(weights, idx_list, sizes, n, dtype):
    vals, pairs, lens, margin = [], [], [], np.inf
    lo = 0
    for e, size in zip(idx_list, sizes):
        trace = []
        v, pr = uref.adjacency_power(torch.from_numpy(weights[lo:lo + len(e)]).to(dtype), e, size, n, trace)
        lo += len(e)
        power, reach = trace[0]
        if reach.any():
            margin = min(margin, float(np.abs(power[reach] - uref.EPS).min()))
        vals.append(v.numpy())
        pairs.append(pr.reshape(-1, 2))
        lens.append(len(pr))
    return np.concatenate(vals), np.concatenate(pairs), _splits(lens), margin


def _run_power(weights, idx_list, sizes, n, node_indexing="sample", extra_columns=0):
    from gcnn_keras_amd.layers.pool.topk import AdjacencyPower
    ns, es = _splits(sizes), _splits([len(e) for e in idx_list])
    flat = np.concatenate([e.reshape(-1, 2) for e in idx_list]).astype(np.int64)
    if node_indexing == "batch":
        flat = flat + np.repeat(ns[:-1], np.diff(es))[:, None]
    w = weights
    if extra_columns:   # column 0 alone is read
        w = np.concatenate([weights, np.full((len(weights), extra_columns), 1e3, np.float32)], axis=1)
    nodes = _rag(np.zeros((int(ns[-1]), 2), np.float32), ns)
    with torch.no_grad():
        edges_out, idx_out = AdjacencyPower(n=n, node_indexing=node_indexing)([nodes, _rag(w, es), _rag(flat, es)])
    return edges_out, idx_out, nodes, ns


def _small_power_batch():
    """Integer weights, exact in both precisions: a path; one node with a self loop; +1 / -1 that cancel exactly; a
    negative product beside a positive one; a graph without nodes; a node without edges."""
    idx = [np.array([[0, 1], [1, 2], [2, 3]]), np.array([[0, 0]]),
           np.array([[0, 1], [0, 2], [1, 3], [2, 3], [3, 0]]), np.array([[2, 0], [0, 1], [1, 2], [0, 0]]),
           np.zeros((0, 2)), np.zeros((0, 2))]
    w = [[2, 3, 5], [3], [1, 1, 1, -1, -2], [-2, 3, 1, -1], [], []]
    sizes = [4, 1, 4, 3, 0, 1]
    idx = [np.asarray(e, dtype=np.int64) for e in idx]
    return np.concatenate([np.asarray(v, dtype=np.float32) for v in w]).reshape(-1, 1), idx, sizes


@pytest.mark.parametrize("node_indexing", ["sample", "batch"])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_adjacency_power_exact_cases(n, node_indexing):
    w, idx_list, sizes = _small_power_batch()
    vals, pairs, splits, _ = _power_reference(w, idx_list, sizes, n, torch.float64)
    edges_out, idx_out, nodes, ns = _run_power(w, idx_list, sizes, n, node_indexing, extra_columns=2)
    got_pairs, got_splits = _host(idx_out)
    if node_indexing == "batch":
        pairs = pairs + np.repeat(ns[:-1], np.diff(splits))[:, None]
    assert np.array_equal(got_splits, splits) and np.array_equal(_host(edges_out)[1], splits)
    assert np.array_equal(got_pairs, pairs)
    assert np.array_equal(_host(edges_out)[0], vals.astype(np.float32))      # integers: exact
    if n == 2:
        # the path gives (0,2) = 6 and (1,3) = 15; the self loop 9; the cancelled (0,3) and the negative entries are gone
        assert vals[:3, 0].tolist() == [6.0, 15.0, 9.0]
        g2 = pairs[splits[2]:splits[3]] - (ns[2] if node_indexing == "batch" else 0)
        assert g2.tolist() == [[2, 0]]


@functools.lru_cache(maxsize=None)
def _random_power_case(name):
    rng = np.random.default_rng(17)
    if name == "cora":
        c = synth.cora_like_graph()
        idx_list, sizes = [c["edge_indices"]], [int(c["node_splits"][-1])]
    else:
        sizes = [1, 65, 300]
        idx_list = _ring_edges(rng, sizes, extra=2, shuffle=True, loops=True)
    m = sum(len(e) for e in idx_list)
    w = rng.uniform(0.5, 1.5, size=(m, 1)).astype(np.float32)
    return w, idx_list, sizes


@pytest.mark.parametrize("name,n", [("sizes", 1), ("sizes", 2), ("sizes", 3), ("cora", 2)])
def test_adjacency_power_random_weights(name, n):
    """Graphs of 1, 65 and 300 nodes (unsorted lists with self loops) and one Cora-like graph of 2708 nodes - more than
    one column range of the row accumulator - with weights in [0.5, 1.5): every entry a product can reach is at least
    0.125, far from the threshold (asserted), so the index lists have one answer."""
    w, idx_list, sizes = _random_power_case(name)
    v64, p64, s64, margin = _power_reference(w, idx_list, sizes, n, torch.float64)
    v32, p32, s32, _ = _power_reference(w, idx_list, sizes, n, torch.float32)
    assert margin >= 1e-4 and np.array_equal(p32, p64)
    assert max(sizes) > _ffi.MP_TOPK_ACC_FLOATS or name != "cora"
    edges_out, idx_out, nodes, _ = _run_power(w, idx_list, sizes, n)
    again, _, _, _ = _run_power(w, idx_list, sizes, n)
    got_pairs, got_splits = _host(idx_out)
    assert np.array_equal(got_splits, s64) and np.array_equal(got_pairs, p64)
    assert_rows_close(_host(edges_out)[0], v32, v64, what="A^%d %s" % (n, name))
    assert torch.equal(edges_out.values, again.values)                        # equal bits on every call
    plan = idx_out.index_plan(nodes)                                          # the attached plan is a fresh one's
    fresh = _rag(got_pairs, got_splits).index_plan(nodes)
    assert torch.equal(plan.cols[:, :plan.M], fresh.cols[:, :fresh.M]) and torch.equal(plan.csr(0)[0], fresh.csr(0)[0])


def test_adjacency_power_refuses_a_gradient_in_the_edges():
    from gcnn_keras_amd.layers.pool.topk import AdjacencyPower
    w, idx_list, sizes = _small_power_batch()
    ns, es = _splits(sizes), _splits([len(e) for e in idx_list])
    edges = _rag(w, es)
    edges.values.requires_grad_(True)
    with pytest.raises(NotImplementedError):
        AdjacencyPower()([_rag(np.zeros((int(ns[-1]), 1), np.float32), ns), edges, _rag(np.concatenate(idx_list), es)])


# ------------------------------------------------------------------------------------------------ unpool
def _pool_unpool_inputs(k):
    rng = np.random.default_rng(5)
    sizes = [0, 1, 5, 15, 65, 0]
    ns = _splits(sizes)
    x = rng.integers(-3, 4, size=(int(ns[-1]), 4)).astype(np.float32)
    idx_list = _ring_edges(rng, sizes)
    es = _splits([len(e) for e in idx_list])
    edges = rng.normal(size=(int(es[-1]), 3)).astype(np.float32)
    return [_rag(x, ns), _rag(edges, es), _rag(np.concatenate(idx_list), es)], x, edges


@pytest.mark.parametrize("k", [0.3, 1.0])
def test_unpool_round_trip(k):
    """``k = 1.0`` keeps nothing: the un-pooled tensors are zeros of the old shapes.  Otherwise the kept rows return to
    their places (as the pooled, gated rows) and everything else is zero; maps rebuilt from their values alone (no
    inverse table attached) give the same."""
    from gcnn_keras_amd.layers.pool.topk import PoolingTopK, UnPoolingTopK
    inputs, x, edges = _pool_unpool_inputs(k)
    with torch.no_grad():
        pooled, maps = PoolingTopK(k=k, kernel_initializer="ones")(inputs)
        out = UnPoolingTopK()(inputs + maps + pooled)
        bare = [_rag(*_host(m)) for m in maps]
        out_bare = UnPoolingTopK()(inputs + bare + pooled)
    ns, es = inputs[0].row_splits_host(), inputs[1].row_splits_host()
    for got, old, pool_t, map_t, splits in ((out[0], x, pooled[0], maps[0], ns), (out[1], edges, pooled[1], maps[1], es)):
        vals = got.values.cpu().numpy()
        assert vals.shape == (old.shape[0], pool_t.values.shape[1]) and np.array_equal(_host(got)[1], splits)
        want = np.zeros_like(vals)
        mv, ms = _host(map_t)
        where = mv + np.repeat(splits[:-1], np.diff(ms))
        want[where] = pool_t.values.cpu().numpy()
        assert np.array_equal(vals, want)
        if k == 1.0:
            assert len(mv) == 0 and not vals.any()
    assert out[2] is inputs[2]
    for a, b in zip(out[:2], out_bare[:2]):
        assert torch.equal(a.values, b.values)


def test_unpool_with_skip_is_unpool_plus_add():
    from gcnn_keras_amd.layers.modules import LazyAdd
    from gcnn_keras_amd.layers.pool.topk import PoolingTopK, UnPoolingTopK
    inputs, x, _ = _pool_unpool_inputs(0.3)
    with torch.no_grad():
        pooled, maps = PoolingTopK(k=0.3, kernel_initializer="ones")(inputs)
        before = _ffi.launch_count()
        fused = UnPoolingTopK().call_with_skip(inputs + maps + pooled, inputs[0], with_edges=False)
        assert _ffi.launch_count() - before == 1                  # one launch for scatter + skip
        two = UnPoolingTopK()(inputs + maps + pooled)
        want = LazyAdd()([two[0], inputs[0]])
    assert torch.equal(fused[0].values, want.values)
    assert fused[1] is inputs[1]


# ------------------------------------------------------------------------------------------------ the model
def _model_inputs(b, graphs=None):
    ns, es = b["node_splits"], b["edge_splits"]
    if graphs is not None:
        ns, es = ns[:graphs + 1], es[:graphs + 1]
    return ([_rag(b["node_attributes"][:ns[-1]], ns), _rag(b["edge_weights"][:es[-1]], es),
             _rag(b["edge_indices"][:es[-1]], es)],
            {"nodes": b["node_attributes"][:ns[-1]], "edges": b["edge_weights"][:es[-1]],
             "edge_indices": b["edge_indices"][:es[-1]], "node_splits": ns, "edge_splits": es})


@functools.lru_cache(maxsize=None)
def _model_case(use_reconnect, output_embedding):
    """Model, device inputs and both restatements on the 12 committed graphs (tests/test_unet_api.py asserts the input
    conditions for them)."""
    from gcnn_keras_amd.literature import Unet
    model = Unet.make_model(inputs=FEATURE_INPUTS, use_reconnect=use_reconnect, output_embedding=output_embedding,
                            output_to_tensor=False)
    params = synth.unet_params(model)
    model.set_weights(list(params.values()))
    inputs, batch = _model_inputs(synth.unet_batch(12))
    refs = {}
    for dt in (torch.float32, torch.float64):
        w = [torch.from_numpy(v).to(dt) for v in params.values()]
        refs[dt] = uref.unet_forward(w, batch, use_reconnect=use_reconnect, output_embedding=output_embedding,
                                     dtype=dt).numpy()
    return model, params, inputs, refs


@pytest.mark.parametrize("output_embedding", ["graph", "node"])
@pytest.mark.parametrize("use_reconnect", [True, False])
def test_model_forward(use_reconnect, output_embedding):
    model, _, inputs, refs = _model_case(use_reconnect, output_embedding)
    with torch.no_grad():
        out = model(inputs)
        again = model(inputs)
    got = (out.values if output_embedding == "node" else out).cpu().numpy()
    assert model.last_route == "eager"
    assert_rows_close(got, refs[torch.float32], refs[torch.float64],
                      what="Unet reconnect=%s %s" % (use_reconnect, output_embedding))
    assert torch.equal(out.values if output_embedding == "node" else out,
                       again.values if output_embedding == "node" else again)


def test_dense_in_front_of_the_gather_gives_the_bits_of_the_edge_side_order():
    from gcnn_keras_amd.layers.gather import GatherNodesOutgoing
    model, _, inputs, _ = _model_case(True, "graph")
    dense = model.layers[3]
    rng = np.random.default_rng(3)
    n = _rag(rng.normal(size=(int(inputs[0].values.shape[0]), 32)).astype(np.float32), inputs[0].row_splits_host())
    with torch.no_grad():
        node_side = GatherNodesOutgoing()([dense(n), inputs[2]])
        edge_side = dense(GatherNodesOutgoing()([n, inputs[2]]))
    assert torch.equal(node_side.values, edge_side.values)


def test_model_gradients_of_all_weights():
    """4 graphs, a fixed linear functional of the output: every weight's gradient against autograd through the
    restatement (the selection is a constant in both).  Each gradient tensor is judged as one row."""
    from gcnn_keras_amd.literature import Unet
    model = Unet.make_model(inputs=FEATURE_INPUTS)
    params = synth.unet_params(model)
    model.set_weights(list(params.values()))
    inputs, batch = _model_inputs(synth.unet_batch(12), graphs=4)
    coeff = np.random.default_rng(9).normal(size=(4, 1))
    refs = {}
    for dt in (torch.float32, torch.float64):
        w = [torch.from_numpy(v).to(dt).requires_grad_(True) for v in params.values()]
        out = uref.unet_forward(w, batch, dtype=dt)
        (out * torch.from_numpy(coeff).to(dt)).sum().backward()
        refs[dt] = [t.grad.numpy() for t in w]
    model.requires_grad_(True)
    try:
        with torch.enable_grad():
            out = model(inputs)
            (out * torch.from_numpy(coeff).float().cuda()).sum().backward()
        grads = [t.grad for t in model.trainable_weights]
    finally:
        model.requires_grad_(False)
    for (name, t), g, r32, r64 in zip(model.weights, grads, refs[torch.float32], refs[torch.float64]):
        assert g is not None, name
        assert np.abs(r64).max() > 0, name
        assert_rows_close(g.cpu().numpy().reshape(1, -1), r32.reshape(1, -1), r64.reshape(1, -1), what="d/d " + name)
        t.grad = None


def test_train_on_batch_lowers_the_loss_on_the_default_model():
    from gcnn_keras_amd.literature import Unet
    model = Unet.make_model()
    model.set_weights(list(synth.unet_params(model).values()))
    b = synth.unet_batch(12)
    x = [_rag(b["node_number"], b["node_splits"]), _rag(b["edge_number"], b["edge_splits"]),
         _rag(b["edge_indices"], b["edge_splits"])]
    y = torch.from_numpy((np.arange(12) % 2).astype(np.float32).reshape(12, 1)).cuda()
    model.compile(optimizer="adam", loss="binary_crossentropy")
    first = model.train_on_batch(x, y)
    second = model.train_on_batch(x, y)
    assert np.isfinite(first) and second < first
    assert model.weights[1][1].grad is None          # the edge embedding is off the tape (Unet.py docstring)
