"""MEGNet for crystals on the engine (csrc/mp_megnet.hip, literature/Megnet.make_crystal_model): the fused edge step of a
``MEGnetBlock`` against the layer sequence and against the torch restatement (tests/megnet_reference.py, float32 with the
float64 twin as budget) on graphs that put receivers and graphs inside, across and over whole tiles of 32 edges; the
crystal model (eager, replayed, ``predict``, shuffled lists, given distances, ``SetRangePeriodic`` output); training through
the layer sequence and the guards.

Two layer-level cases end in a graph without edges (``hand0``: the only graph has none; ``multi7``).  The per-graph edge
pool of the layers follows the reference's segment ops, which drop trailing empty graphs, so the state chain's
concatenation meets ``G - 1`` edge-pool rows and raises ``ValueError`` - on both routes, since both run the state chain on
the same layers.  For these two the block-level check is that the fused block raises what the layer sequence raises; the
fused step's own outputs (``e'`` and the receiver pool) are still held against the restatement."""
import os

import numpy as np
import pytest
import torch

import megnet_reference as ref
import periodic_reference as pr
from gcnn_keras_amd import _ffi, synth
from gcnn_keras_amd.layers.conv.megnet_conv import MEGnetBlock
from gcnn_keras_amd.literature import Megnet
from gcnn_keras_amd.ragged import RaggedTensor
from parity import assert_rows_close, rowwise_rel

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CASES = {}


def cases():
    if not _CASES:
        _CASES.update(pr.golden_cases(GOLDEN))
    return _CASES


def _rag(values, splits):
    return RaggedTensor.from_numpy(np.ascontiguousarray(values), splits)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ fused edge step
CONFIGS = {
    "softplus2_mean_bias": dict(activation="kgcnn>softplus2", pooling_method="mean", use_bias=True),
    "swish_sum_nobias": dict(activation="swish", pooling_method="sum", use_bias=False),
}
GOLDEN_GRAPHS = ["thin2_c40", "cubic1_c40", "big6_c40", "tri5_c40", "tri5_c55"]
HAND_GRAPHS = ["hand0", "hand1", "hand31", "hand32", "hand33", "hand64", "hand65"]
GRAPHS = GOLDEN_GRAPHS + HAND_GRAPHS + ["multi", "multi_shuffled", "graphs2100"]
ENDS_WITHOUT_EDGES = ("hand0", "multi7")     # the module docstring


def graph_case(name, seed=0):
    """``(v (N, 32), e (E, 32), u (G, 32), edge_indices, node_splits, edge_splits)`` of a named layer-level case: random
    normal features, so a wrong graph id shows far above the bar."""
    if name.startswith("hand"):
        idx, ns, es = ref.hand_case(int(name[4:]), seed)
    elif name == "graphs2100":      # past the 2048 graphs whose row splits the kernel keeps in LDS
        idx, ns, es = ref.many_graphs_case(2100)
    elif name.startswith("multi"):
        idx, ns, es = ref.multi_case(seed, shuffled=name == "multi_shuffled", graphs=7 if name == "multi7" else 8)
    else:
        c = cases()[name]
        idx, ns, es = c["indices"], np.array([0, len(c["xyz"])]), np.array([0, len(c["indices"])])
    rng = np.random.default_rng(seed + 100)
    n, e, g = int(ns[-1]), int(es[-1]), len(ns) - 1
    return (rng.normal(size=(n, 32)).astype(np.float32), rng.normal(size=(e, 32)).astype(np.float32),
            rng.normal(size=(g, 32)).astype(np.float32), np.asarray(idx, np.int64).reshape(-1, 2), ns, es)


def make_block(seed, **kwargs):
    rng = np.random.default_rng(seed)
    blk = MEGnetBlock(node_embed=[64, 32, 32], edge_embed=[64, 32, 32], env_embed=[64, 32, 32], **kwargs)
    blk.ensure_built([(None, None, 32), (None, None, 32), (None, None, 2), (None, 32)])
    ws = []
    for name, t in blk.weights:
        shape = tuple(t.shape)
        ws.append(synth.glorot_uniform(rng, shape[0], shape[1], shape=shape) if name.endswith("kernel")
                  else rng.uniform(-0.1, 0.1, shape))
    blk.set_weights([np.asarray(w, np.float32) for w in ws])
    return blk


def _ref_block(blk, v, e, u, flat, ns, es, dtype):
    it = iter([torch.tensor(w, dtype=dtype) for w in blk.get_weights()])
    w = ref.take_block_weights(it, blk.use_bias)
    out = ref.megnet_block(torch.tensor(v, dtype=dtype), torch.tensor(e, dtype=dtype), torch.from_numpy(flat),
                           torch.tensor(u, dtype=dtype), ref.graph_ids(ns), ref.graph_ids(es), w,
                           blk.lay_phi_e.activation, blk.pooling_method)
    pool = ref.seg_pool(out[1], torch.from_numpy(flat)[:, 0], len(v), blk.pooling_method)
    return [t.numpy() for t in out] + [pool.numpy()]


def _outcome(fn):
    """The values of ``fn()`` or the exception it raises."""
    try:
        return fn(), None
    except Exception as err:      # noqa: BLE001 - the kind of exception is what is compared
        return None, err


def check_edge_case(name, config, seed=0):
    v, e, u, idx, ns, es = graph_case(name, seed)
    blk = make_block(seed + 1, **CONFIGS[config])
    assert blk.fused_edge is True
    x = [_rag(v, ns), _rag(e, es), _rag(idx, es), _cuda(u)]
    what = "edge step %s %s" % (name, config)
    flat = ref.flat_edges({"edge_indices": idx, "node_splits": ns, "edge_splits": es})
    r32, r64 = (_ref_block(blk, v, e, u, flat, ns, es, dt) for dt in (torch.float32, torch.float64))
    with torch.no_grad():
        # the fused step by itself: e' in list order and the pool into the receivers
        ep, pool = blk._fused_step(*x)
        ep2, pool2 = blk._fused_step(*x)
        assert torch.equal(ep.values, ep2.values) and torch.equal(pool.values, pool2.values)
        pooled_by_layer = blk.lay_esum([x[0], ep, x[2]]).values
    assert tuple(ep.values.shape) == (len(e), 32) and tuple(pool.values.shape) == (len(v), 32)
    if len(e):           # parity.py takes no tensor without rows: an empty e' is held to its shape, asserted above
        assert_rows_close(ep.values.cpu().numpy(), r32[1], r64[1], what=what + " e' (step)")
    assert_rows_close(pool.values.cpu().numpy(), r32[3], r64[3], what=what + " pool (step)")
    assert_rows_close(pool.values.cpu().numpy(), pooled_by_layer.cpu().numpy(), what=what + " pool vs PoolingLocalEdges")
    lone = np.bincount(flat[:, 0], minlength=len(v)) == 0
    assert np.all(pool.values.cpu().numpy()[lone] == 0.0)              # receivers without edges pool to exactly 0

    def run():
        with torch.no_grad():
            return [t.values if isinstance(t, RaggedTensor) else t for t in blk(x)]

    launches = _ffi.launch_count()
    fused, fused_err = _outcome(run)
    fused_launches = _ffi.launch_count() - launches
    blk.use_fused_edge = False
    launches = _ffi.launch_count()
    seq, seq_err = _outcome(run)
    seq_launches = _ffi.launch_count() - launches
    blk.use_fused_edge = True
    if name in ENDS_WITHOUT_EDGES:
        # exactly what the layer sequence does: the same shapes or the same exception
        assert (fused_err is None) == (seq_err is None)
        if seq_err is not None:
            assert type(fused_err) is type(seq_err) and str(fused_err) == str(seq_err)
        else:
            assert [tuple(t.shape) for t in fused] == [tuple(t.shape) for t in seq]
        return lone
    assert fused_err is None and seq_err is None, (fused_err, seq_err)
    again = run()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        other = run()
    s.synchronize()
    for a, b, c in zip(fused, again, other):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert fused_launches < seq_launches                      # the fused kernel ran, not the layer sequence
    for k, label in enumerate(("v'", "e'", "u'")):
        got, lay = fused[k].cpu().numpy(), seq[k].cpu().numpy()
        assert got.shape == r64[k].shape
        assert_rows_close(got, r32[k], r64[k], what="%s %s" % (what, label))
        assert_rows_close(lay, r32[k], r64[k], what="%s %s (layer sequence)" % (what, label))
        bar = max(1e-5, min(2 * rowwise_rel(r32[k], r64[k]), 5e-5))
        err = rowwise_rel(got, lay)
        assert err <= 2 * bar, "%s %s: fused vs layer sequence %.3g" % (what, label, err)
    return lone


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("name", GRAPHS)
def test_fused_edge_step_graphs(name, config):
    lone = check_edge_case(name, config)
    if name == "big6_c40" or name.startswith("hand") or name.startswith("multi") or name == "graphs2100":
        assert lone.any()


@pytest.mark.parametrize("config", list(CONFIGS))
def test_batch_ending_in_an_edgeless_graph_does_what_the_layer_sequence_does(config):
    check_edge_case("multi7", config)


def test_every_activation_code_runs_the_dense_epilogue_function():
    v, e, u, idx, ns, es = graph_case("multi")
    x = [_rag(v, ns), _rag(e, es), _rag(idx, es), _cuda(u)]
    for act in ("relu", "kgcnn>shifted_softplus", "softplus", "sigmoid", "tanh", "kgcnn>leaky_relu", "selu", "linear"):
        blk = make_block(3, activation=act)
        assert blk.fused_edge is True
        with torch.no_grad():
            fused = blk(x)[1].values
            blk.use_fused_edge = False
            seq = blk(x)[1].values
        assert_rows_close(fused.cpu().numpy(), seq.cpu().numpy(), what="edge step, activation %s" % act)


# ------------------------------------------------------------------------------------------------ guards
def test_fused_edge_step_guards():
    v, e, u, idx, ns, es = graph_case("thin2_c40")
    blk = make_block(1)
    x = [_rag(v, ns), _rag(e, es), _rag(idx, es), _cuda(u)]
    with torch.no_grad():
        launches = _ffi.launch_count()
        base = [t.values if isinstance(t, RaggedTensor) else t for t in blk(x)]
        fused_launches = _ffi.launch_count() - launches
        blk.use_fused_edge = False
        seq = [t.values if isinstance(t, RaggedTensor) else t for t in blk(x)]
        blk.use_fused_edge = True
    # any tape takes the layer sequence and gives the values of use_fused_edge=False: an input that requires grad ...
    vv = _cuda(v).requires_grad_(True)
    with torch.enable_grad():
        launches = _ffi.launch_count()
        out = blk([x[0].with_values(vv), x[1], x[2], x[3]])
        assert _ffi.launch_count() - launches > fused_launches
        (v_bar,) = torch.autograd.grad(out[1].values.sum() + out[2].sum(), [vv])
    # the tape's Dense saves its pre-activation and may tile differently from the plain one: the same float32 formulas,
    # held to 2e-6 (a few ulp over the block's three chains; parity.py asks no pipeline for less)
    for a, b in zip(out, seq):
        a = a.values if isinstance(a, RaggedTensor) else a
        assert_rows_close(a.detach().cpu().numpy(), b.cpu().numpy(), rtol=2e-6, what="layer sequence on a tape")
    assert float(v_bar.abs().max()) > 0
    # ... the state, or a weight
    uu = _cuda(u).requires_grad_(True)
    with torch.enable_grad():
        out = blk([x[0], x[1], x[2], uu])
        (u_bar,) = torch.autograd.grad(out[1].values.sum(), [uu])
    assert_rows_close(out[1].values.detach().cpu().numpy(), seq[1].cpu().numpy(), rtol=2e-6, what="state on a tape")
    assert float(u_bar.abs().max()) > 0
    blk.lay_phi_e_2.kernel.requires_grad_(True)
    try:
        with torch.enable_grad():
            out = blk(x)
            (k_bar,) = torch.autograd.grad(out[0].values.sum(), [blk.lay_phi_e_2.kernel])
        assert_rows_close(out[1].values.detach().cpu().numpy(), seq[1].cpu().numpy(), rtol=2e-6, what="weight on a tape")
        assert float(k_bar.abs().max()) > 0
        with torch.no_grad():
            assert torch.equal(blk(x)[1].values, base[1])          # no tape: the fused step, whatever the weights say
    finally:
        blk.lay_phi_e_2.kernel.requires_grad_(False)
    # keyword arguments take the layer sequence too
    with torch.no_grad():
        launches = _ffi.launch_count()
        blk(x, training=False)
        assert _ffi.launch_count() - launches > fused_launches
    # out-of-range edges raise before the kernel runs
    bad = idx.copy()
    bad[3, 1] = 7
    with pytest.raises(IndexError), torch.no_grad():
        blk([x[0], x[1], _rag(bad, es), x[3]])
    # widths the kernel does not serve are refused by the C call, not computed wrongly
    with pytest.raises(ValueError, match="mp_megnet_edge_f32"):
        _ffi.call("mp_megnet_edge_f32", *([None] * 2 + [4, None, None, 1, None, 16, 32, 32, None, 0] + [None] * 7
                                          + [64, 32, 32, 8, 0.05, _ffi.MP_MEAN, None, 0, None, None, None]))


# ------------------------------------------------------------------------------------------------ model
BATCH = ["tri5_c40", "cubic1_c40", "big6_c40", "thin2_c40"]


def crystal_batch(names, state="float", shuffle_seed=None, seed=8):
    """Golden structures as one MEGNet batch; ``state``: ``"float"`` a ``(G, 1)`` charge, ``"int"`` ``(G,)`` numbers for
    the embedding; ``shuffle_seed``: every structure's edge list reordered."""
    rng = np.random.default_rng(seed)
    shuffle = None if shuffle_seed is None else np.random.default_rng(shuffle_seed)
    numbers, xyz, lats, idx, img, dist = [], [], [], [], [], []
    for k, name in enumerate(names):
        c = cases()[name]
        i, m, d = c["indices"], c["images"], c["dist"]
        if shuffle is not None:
            order = shuffle.permutation(len(i))
            i, m, d = i[order], m[order], d[order]
        numbers.append(np.resize(np.array([1, 6, 7, 8, 14], np.float32), len(c["xyz"])) + k % 3)
        xyz.append(c["xyz"]), lats.append(c["lattice"]), idx.append(i), img.append(m), dist.append(d)
    splits = lambda parts: np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    g = len(names)
    return {"node_number": np.concatenate(numbers).astype(np.float32),
            "node_coordinates": np.concatenate(xyz, axis=0).astype(np.float32), "node_splits": splits(xyz),
            "graph_lattice": np.stack(lats).astype(np.float32), "edge_indices": np.concatenate(idx, axis=0).astype(np.int64),
            "edge_image": np.concatenate(img, axis=0).astype(np.int64), "edge_splits": splits(idx),
            "edge_distance": np.concatenate(dist).astype(np.float32).reshape(-1, 1),
            "state": rng.normal(size=(g, 1)).astype(np.float32) if state == "float"
            else rng.integers(0, 100, size=g).astype(np.float32)}


def model_inputs(b, distances=False):
    second = _rag(b["edge_distance"], b["edge_splits"]) if distances else _rag(b["node_coordinates"], b["node_splits"])
    return [_rag(b["node_number"], b["node_splits"]), second, _rag(b["edge_indices"], b["edge_splits"]),
            _cuda(b["state"]), _rag(b["edge_image"], b["edge_splits"]), _cuda(b["graph_lattice"])]


def random_params(model, seed):
    """Glorot kernels, biases in +-0.1, embeddings in +-0.05 (``synth.cgcnn_params`` draws by weight name)."""
    return list(synth.cgcnn_params(model, seed=seed).values())


def _model(state="float", seed=21, **cfg):
    if state == "int":
        inputs = list(Megnet.model_crystal_default["inputs"])
        inputs[3] = {"shape": [], "name": "charge", "dtype": "float32", "ragged": False}
        cfg = dict(cfg, inputs=inputs)
    m = Megnet.make_crystal_model(**cfg)
    p = random_params(m, seed)
    m.set_weights(p)
    return m, p


_REFS = {}


def _refs(key, p, b, cfg):
    """float32 and float64 restatement outputs, computed once per (model, batch) key."""
    if key not in _REFS:
        _REFS[key] = tuple(ref.megnet_forward(p, b, cfg, dtype=dt).numpy() for dt in (torch.float32, torch.float64))
    return _REFS[key]


@pytest.mark.parametrize("state", ["float", "int"])
def test_crystal_model_defaults_match_restatement(state):
    b = crystal_batch(BATCH, state)
    m, p = _model(state)
    assert m.fused_edge_blocks == [True] * 3 and m.config["use_set2set"] is True
    r32, r64 = _refs(("default", state), p, b, m.config)
    x = model_inputs(b)
    with torch.no_grad():
        eager = m(x)
        assert m.last_route == "eager"
        second, third = m(x), m(x)
        assert m.last_route == "graph"
        served = m.predict(x, batch_size=2)
        m.use_fused_edge = False
        seq = m(x)
        assert m.last_route == "eager"                       # flipping the switch dropped the captured graphs
        m.use_fused_edge = True
    assert tuple(eager.shape) == (4, 1)
    assert torch.equal(eager, second) and torch.equal(eager, third)
    assert_rows_close(eager.cpu().numpy(), r32, r64, what="MEGNet crystal defaults (%s state), fused" % state)
    assert_rows_close(third.cpu().numpy(), r32, r64, what="MEGNet crystal defaults (%s state), replayed" % state)
    assert_rows_close(served.cpu().numpy(), r32, r64, what="MEGNet crystal defaults (%s state), predict" % state)
    assert_rows_close(seq.cpu().numpy(), r32, r64, what="MEGNet crystal defaults (%s state), layer sequence" % state)
    # shuffled edge lists: the plan's permutation serves the fused step; the output is that of the sorted lists
    bs = crystal_batch(BATCH, state, shuffle_seed=6)
    with torch.no_grad():
        shuffled = m(model_inputs(bs))
    s32, s64 = _refs(("default-shuffled", state), p, bs, m.config)
    assert_rows_close(shuffled.cpu().numpy(), s32, s64, what="MEGNet crystal defaults (%s state), shuffled" % state)
    assert_rows_close(shuffled.cpu().numpy(), r32, r64, what="MEGNet crystal defaults (%s state), shuffled vs sorted" % state)


def test_given_distances_equal_the_coordinate_route():
    b = crystal_batch(BATCH)
    m, p = _model()
    r32, r64 = _refs(("default", "float"), p, b, m.config)
    inputs = list(Megnet.model_crystal_default["inputs"])
    inputs[1] = {"shape": (None, 1), "name": "edge_distance", "dtype": "float32", "ragged": True}
    md, _ = _model(make_distance=False, inputs=inputs)
    md.set_weights(p)
    with torch.no_grad():
        got = md(model_inputs(b, distances=True))
        short = md(model_inputs(b, distances=True)[:4])      # the image and the lattice are not read
    assert torch.equal(got, short)
    assert_rows_close(got.cpu().numpy(), r32, r64, what="MEGNet crystal, make_distance=False")


def test_set_range_periodic_output_feeds_the_model():
    from gcnn_keras_amd.graph.preprocessor import SetRangePeriodic
    b = crystal_batch(BATCH)
    assert all(cases()[n]["cutoff"] == 4.0 and cases()[n]["maxn"] is None for n in BATCH)
    m, p = _model()
    r32, r64 = _refs(("default", "float"), p, b, m.config)
    x = model_inputs(b)
    lattice = x[5]
    idx, img, dist = SetRangePeriodic(max_distance=4.0)(x[1], lattice)
    assert img.values.dtype == torch.int64 and int(idx.values.shape[0]) == len(b["edge_indices"])
    with torch.no_grad():
        got = m([x[0], x[1], idx, x[3], img, lattice])        # range_indices / range_image / lattice as they come
        golden = m(x)
    assert_rows_close(got.cpu().numpy(), r32, r64, what="MEGNet on SetRangePeriodic output")
    assert_rows_close(got.cpu().numpy(), golden.cpu().numpy(), what="SetRangePeriodic output vs the golden lists")


def test_stale_weights_and_the_switch():
    b = crystal_batch(BATCH)
    m, _ = _model()
    x = model_inputs(b)
    with torch.no_grad():
        first = m(x)
        m(x)
        assert torch.equal(m(x), first) and m.last_route == "graph"
    # weights changed in place: the replayed graph reads them where they are (the fused step keeps no repacked copy)
    m.set_weights([0.5 * w for w in m.get_weights()])
    with torch.no_grad():
        replayed = m(x)
        assert m.last_route == "graph"
        m.auto_graph = False
        eager = m(x)
        m.auto_graph = True
    assert torch.equal(replayed, eager) and not torch.equal(replayed, first)
    # the switch drops the captured graphs: the next call runs the layer sequence, not a replay of the fused route
    m.use_fused_edge = False
    with torch.no_grad():
        seq = m(x)
    assert m.last_route == "eager"
    m.use_fused_edge = True
    assert_rows_close(seq.cpu().numpy(), eager.cpu().numpy(), what="layer sequence after the switch")
    # the per-block switch is part of a captured graph's identity too
    m.blocks[1].use_fused_edge = False
    with torch.no_grad():
        m(x)
    assert m.last_route == "eager" and m.use_fused_edge is False
    m.blocks[1].use_fused_edge = True


def test_molecular_builder_takes_the_fused_route_too():
    b = synth.qm9_like_batch(num_graphs=5, seed=41)
    b["state"] = np.array([3, 0, 7, 99, 5], np.float32)
    m = Megnet.make_model()
    p = random_params(m, 4)
    m.set_weights(p)
    assert m.fused_edge_blocks == [True] * 3
    x = [_rag(b["node_number"], b["node_splits"]), _rag(b["node_coordinates"], b["node_splits"]),
         _rag(b["edge_indices"], b["edge_splits"]), _cuda(b["state"])]
    with torch.no_grad():
        launches = _ffi.launch_count()
        got = m(x)
        fused_launches = _ffi.launch_count() - launches
        m.use_fused_edge = False
        launches = _ffi.launch_count()
        seq = m(x)
        seq_launches = _ffi.launch_count() - launches
    assert fused_launches < seq_launches
    r32, r64 = (ref.megnet_forward(p, b, m.config, dtype=dt, crystal=False).numpy() for dt in (torch.float32, torch.float64))
    assert_rows_close(got.cpu().numpy(), r32, r64, what="Megnet.make_model, fused")
    assert_rows_close(seq.cpu().numpy(), r32, r64, what="Megnet.make_model, layer sequence")


# ------------------------------------------------------------------------------------------------ training
def test_gather_state_carries_its_reverse_rule():
    """The state repeat on a tape: the values of the plain call, and the per-graph sum as its reverse (an edgeless graph
    gets a zero gradient row)."""
    from gcnn_keras_amd.layers.gather import GatherState
    rng = np.random.default_rng(11)
    es = np.array([0, 5, 5, 32, 33])
    u = rng.normal(size=(4, 32)).astype(np.float32)
    g = rng.normal(size=(33, 32)).astype(np.float32)
    target = _rag(np.zeros((33, 3), np.float32), es)
    lay = GatherState()
    with torch.no_grad():
        plain = lay([_cuda(u), target]).values
    uu = _cuda(u).requires_grad_(True)
    with torch.enable_grad():
        out = lay([uu, target]).values
        (u_bar,) = torch.autograd.grad(out, [uu], _cuda(g))
    assert torch.equal(out.detach(), plain) and np.array_equal(plain.cpu().numpy(), np.repeat(u, np.diff(es), axis=0))
    want = {dt: np.stack([g[a:b].astype(dt).sum(axis=0) for a, b in zip(es[:-1], es[1:])]) for dt in (np.float32, np.float64)}
    assert_rows_close(u_bar.cpu().numpy(), want[np.float32], want[np.float64], what="GatherState reverse")
    assert np.all(u_bar.cpu().numpy()[1] == 0.0)


TRAIN_CFG = dict(use_set2set=False, nblocks=2)


def _mae(pred, target):
    return (pred - target).abs().mean()


def test_weight_gradients_match_restatement_autograd():
    b = crystal_batch(BATCH)
    m, p = _model(**TRAIN_CFG)
    x = model_inputs(b)
    target = np.random.default_rng(4).normal(size=(4, 1)).astype(np.float32)
    m.requires_grad_(True)
    try:
        with torch.enable_grad():
            loss = _mae(m(x), _cuda(target))
            loss.backward()
        grads = [t.grad.detach().cpu().numpy() for t in m.trainable_weights]
    finally:
        m.requires_grad_(False)
        for t in m.trainable_weights:
            t.grad = None
    refs = {}
    for dt in (torch.float32, torch.float64):
        w = [torch.tensor(a, dtype=dt, requires_grad=True) for a in p]
        rl = _mae(ref.megnet_forward(w, b, m.config, dtype=dt), torch.from_numpy(target).to(dt))
        refs[dt] = (float(rl.detach()), [g.numpy() for g in torch.autograd.grad(rl, w)])
    np.testing.assert_allclose(float(loss.detach()), refs[torch.float64][0], rtol=1e-5)
    for (name, _), g, g32, g64 in zip(m.weights, grads, refs[torch.float32][1], refs[torch.float64][1]):
        # 1e-5 of the tensor's scale, raised to the float32 restatement's own distance from float64 where that is larger
        # (a float32 tape cannot do better), capped as in parity.assert_rows_close
        scale = max(float(np.max(np.abs(g64))), 1e-3)
        e32 = float(np.max(np.abs(g32 - g64))) / scale
        err = float(np.max(np.abs(g - g64))) / scale
        print("[training] %s: gradient %.2e of its scale from float64 (float32 restatement %.2e)" % (name, err, e32))
        assert err <= max(1e-5, min(4 * e32, 5e-5)), name
        if np.max(np.abs(g64)) > 0:
            assert np.max(np.abs(g)) > 0, name


def test_sgd_trajectory_fit_and_the_fused_route_afterwards():
    b = crystal_batch(BATCH)
    m, p = _model(**TRAIN_CFG)
    x = model_inputs(b)
    # targets well away from the random model's outputs (|output| < 1): no residual changes sign within the five steps,
    # so the mean absolute error has no kink on the way and float32 follows the float64 trajectory
    target = (3.0 + np.random.default_rng(5).normal(size=(4, 1))).astype(np.float32)
    lr = 1e-3
    m.compile(optimizer=torch.optim.SGD(m.trainable_weights, lr=lr), loss="mean_absolute_error")
    losses = [m.train_on_batch(x, target) for _ in range(5)]
    assert not any(t.requires_grad for t in m.trainable_weights)
    w = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in p]
    opt = torch.optim.SGD(w, lr=lr)
    ref_losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = _mae(ref.megnet_forward(w, b, m.config), torch.from_numpy(target).double())
        loss.backward()
        opt.step()
        ref_losses.append(float(loss.detach()))
    print("[training] engine %s restatement %s" % (losses, ref_losses))
    np.testing.assert_allclose(losses, ref_losses, rtol=1e-5)
    assert len(set(losses)) == 5
    # the fused route serves the trained weights and gives the prediction of the layer sequence
    trained = [t.detach() for t in w]
    r64 = ref.megnet_forward(trained, b, m.config).numpy()
    r32 = ref.megnet_forward(trained, b, m.config, dtype=torch.float32).numpy()
    with torch.no_grad():
        launches = _ffi.launch_count()
        after = m(x).cpu().numpy()
        fused_launches = _ffi.launch_count() - launches
        m.use_fused_edge = False
        launches = _ffi.launch_count()
        seq = m(x).cpu().numpy()
        assert fused_launches < _ffi.launch_count() - launches
        m.use_fused_edge = True
    assert_rows_close(after, r32, r64, what="trained weights, fused")
    assert_rows_close(seq, r32, r64, what="trained weights, layer sequence")
    assert rowwise_rel(after, seq) <= 2 * max(1e-5, min(2 * rowwise_rel(r32, r64), 5e-5))
    history = m.fit(x, target, batch_size=2, epochs=2, seed=1)
    assert len(history.history["loss"]) == 2 and all(np.isfinite(v) for v in history.history["loss"])


def test_training_with_set2set_raises_and_leaves_the_weights():
    b = crystal_batch(BATCH)
    m, _ = _model(nblocks=1)
    assert m.config["use_set2set"] is True
    m.compile(optimizer="sgd", loss="mean_absolute_error")
    before = m.get_weights()
    with pytest.raises(NotImplementedError, match="weight gradients"):
        m.train_on_batch(model_inputs(b), np.zeros((4, 1), np.float32))
    assert not any(t.requires_grad for t in m.trainable_weights)
    assert all(np.array_equal(a, c) for a, c in zip(before, m.get_weights()))
