"""MXMNet on the engine (csrc/mp_mxmnet.hip): the multiplex edge message in both epilogues and the triplet pool, each
fused against the layer sequence against the torch restatement (tests/mxmnet_reference.py, float32 with the float64 twin
as budget), forward and reverse; both layers; the whole model, forces through EnergyForceModel, determinism, replay and
the training guard.  Every bar is ``parity.py``'s."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import mxmnet_reference as ref
from gcnn_keras_amd import synth
from gcnn_keras_amd.layers.conv import mxmnet_conv
from gcnn_keras_amd.layers.conv.mxmnet_conv import MXMGlobalMP, MXMLocalMP
from gcnn_keras_amd.layers.gather import GatherEmbeddingSelection
from gcnn_keras_amd.layers.mlp import GraphMLP
from gcnn_keras_amd.layers.modules import Dense, LazyAdd, LazyConcatenate, LazyMultiply
from gcnn_keras_amd.layers.pooling import PoolingLocalMessages
from gcnn_keras_amd.literature import MXMNet
from gcnn_keras_amd.model.force import EnergyForceModel
from gcnn_keras_amd.ragged import RaggedTensor
from parity import assert_forces_close, assert_rows_close

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64


def _rag(values, splits):
    return RaggedTensor.from_numpy(np.ascontiguousarray(values), splits)


def _splits(lengths):
    return np.concatenate([np.zeros(1, np.int64), np.cumsum(np.asarray(lengths, dtype=np.int64))])


# ------------------------------------------------------------------------------------------------ edge lists
EDGE_LISTS = ["e0", "e1", "e31", "e32", "e33", "star70", "batch", "shuffled"]


@functools.lru_cache(maxsize=None)
def _edge_list(kind):
    """``(node_splits, edge_splits, edge_indices local to each graph)``; receiver-sorted per graph but for "shuffled".
    "eK": one graph of 7 nodes and K edges; "star70": node 3 receives 70 edges, so its segment spans three tiles of 32
    positions, nodes 0 and 5 a few, the other 72 none; "batch" / "shuffled": an empty graph, a one-atom graph and two
    molecules."""
    rng = np.random.default_rng(len(kind) * 101 + sum(map(ord, kind)))
    if kind[0] == "e":
        graphs = [(7, rng.integers(0, 7, size=(int(kind[1:]), 2)))]
    elif kind == "star70":
        star = np.stack([np.full(70, 3), 4 + np.arange(70)], axis=1)
        graphs = [(75, np.concatenate([[[0, 1], [0, 74]], star, [[5, 0], [5, 5], [5, 3]]], axis=0))]
    else:
        graphs = [(0, np.zeros((0, 2), np.int64)), (1, np.zeros((0, 2), np.int64)),
                  (5, rng.integers(0, 5, size=(12, 2))), (9, rng.integers(0, 9, size=(40, 2)))]
    out = []
    for n, e in graphs:
        e = np.asarray(e, dtype=np.int64).reshape(-1, 2)
        e = e[np.argsort(e[:, 0], kind="stable")]
        if kind == "shuffled":
            e = e[rng.permutation(len(e))]
        out.append(e)
    return (_splits([n for n, _ in graphs]), _splits([len(e) for e in out]),
            np.concatenate(out, axis=0).reshape(-1, 2))


def _flat(idx, idx_splits, target_splits):
    out = idx.copy()
    for g in range(len(idx_splits) - 1):
        out[idx_splits[g]:idx_splits[g + 1]] += target_splits[g]
    return torch.from_numpy(out)


def _rows(got, r32, r64, what):
    """``parity.assert_rows_close`` on tensors; a tensor without rows (no edges, no triplets) has only its shape."""
    got, r32, r64 = (t.detach().cpu().numpy() for t in (got, r32, r64))
    assert got.shape == r32.shape == r64.shape, what
    if got.size == 0:
        return 0.0
    return assert_rows_close(got, r32, r64, what=what)


def _message_layers(w, ka, gate, seed):
    """A one-layer GraphMLP over [x_i || x_j || a] and the bias-free gate Dense, random kernels and a non-zero bias."""
    rng = np.random.default_rng(seed)
    mlp = GraphMLP([w], activation="swish").ensure_built((None, None, 2 * w + ka))
    kernel = synth.glorot_uniform(rng, 2 * w + ka, w).astype(np.float32)
    bias = rng.uniform(-0.3, 0.3, size=w).astype(np.float32)
    mlp.set_weights([kernel, bias])
    lin, wl = None, None
    if gate:
        lin = Dense(w, use_bias=False, activation="linear").ensure_built((None, None, ka))
        wl = synth.glorot_uniform(rng, ka, w).astype(np.float32)
        lin.set_weights([wl])
    return mlp, lin, kernel, bias, wl


def _sequence(x, a, idx, mlp, lin, method, base):
    """The reference's layers on the existing engine kernels."""
    xi, xj = GatherEmbeddingSelection([0, 1])([x, idx])
    y = mlp(LazyConcatenate()([xi, xj, a]))
    if lin is not None:
        y = LazyMultiply()([lin(a), y])
    if method is None:
        return y.values
    out = PoolingLocalMessages(pooling_method=method)([x, y, idx])
    return (out if base is None else LazyAdd()([out, base])).values


def _engine_message(route, ns, es, ei, xn, an, bn, gn, mlp, lin, method):
    """Output and the gradients of (x, a, base) under the upstream ``gn`` on one engine route."""
    x, a, idx = _rag(xn, ns), _rag(an, es), _rag(ei, es)
    xv, av = x.values.clone().requires_grad_(True), a.values.clone().requires_grad_(True)
    bv = None if bn is None else _rag(bn, ns).values.clone().requires_grad_(True)
    x, a = x.with_values(xv), a.with_values(av)
    base = None if bv is None else x.with_values(bv)
    with torch.enable_grad():
        if route == "fused":
            out = mxmnet_conv._edge_message(mlp, x, a, idx, mlp, lin, method, base=base)
        else:
            out = _sequence(x, a, idx, mlp, lin, method, base)
        loss = (out * torch.from_numpy(gn).to(out.device)).sum()
    leaves = [t for t in (xv, av, bv) if t is not None]
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for t, g in zip(leaves, grads)]
    return [out.detach()] + list(grads)


def _reference_message(dtype, ns, es, ei, xn, an, bn, gn, kernel, bias, wl, method):
    t = lambda v: None if v is None else torch.tensor(v, dtype=dtype)   # noqa: E731
    x, a = t(xn).requires_grad_(True), t(an).requires_grad_(True)
    base = None if bn is None else t(bn).requires_grad_(True)
    out = ref.edge_message(x, a, _flat(ei, es, ns), t(kernel), t(bias), t(wl), "swish", method, base)
    leaves = [v for v in (x, a, base) if v is not None]
    grads = torch.autograd.grad((out * t(gn)).sum(), leaves, allow_unused=True)
    grads = [torch.zeros_like(v) if g is None else g for v, g in zip(leaves, grads)]
    return [out.detach()] + list(grads)


# (gate, base, pooling method; None = the edge epilogue)
VARIANTS = [(True, True, "mean"), (False, False, "sum"), (True, False, "sum"), (False, True, "mean"),
            (True, False, None), (False, False, None)]


@pytest.mark.parametrize("ka", [5, 32, 128])
@pytest.mark.parametrize("w", [32, 64, 128])
def test_edge_message_fused_sequence_restatement(w, ka):
    """Both epilogues, with and without gate and base, sum and mean, forward and reverse, over every edge list."""
    assert mxmnet_conv.fused_step_supported(w, ka, "swish", "mean")
    worst = 0.0
    for k, kind in enumerate(EDGE_LISTS):
        ns, es, ei = _edge_list(kind)
        n, e = int(ns[-1]), int(es[-1])
        rng = np.random.default_rng(1000 * w + 10 * ka + k)
        xn, an = rng.normal(size=(n, w)).astype(np.float32), rng.normal(size=(e, ka)).astype(np.float32)
        for gate, with_base, method in VARIANTS:
            mlp, lin, kernel, bias, wl = _message_layers(w, ka, gate, seed=w + ka)
            bn = rng.normal(size=(n, w)).astype(np.float32) if with_base else None
            gn = rng.normal(size=(n if method else e, w)).astype(np.float32)
            fused = _engine_message("fused", ns, es, ei, xn, an, bn, gn, mlp, lin, method)
            seq = _engine_message("sequence", ns, es, ei, xn, an, bn, gn, mlp, lin, method)
            r32 = _reference_message(F32, ns, es, ei, xn, an, bn, gn, kernel, bias, wl, method)
            r64 = _reference_message(F64, ns, es, ei, xn, an, bn, gn, kernel, bias, wl, method)
            names = ["out", "x_bar", "a_bar"] + (["base_bar"] if with_base else [])
            for name, f, s, a32, a64 in zip(names, fused, seq, r32, r64):
                what = "W=%d Ka=%d %s gate=%s base=%s %s %s" % (w, ka, kind, gate, with_base, method, name)
                assert tuple(f.shape) == tuple(a64.shape), what
                worst = max(worst, _rows(f, a32, a64, "fused " + what), _rows(s, a32, a64, "sequence " + what))
                _rows(f, s, a64, "fused against sequence " + what)
            if method and e:   # receivers without edges: base, or exactly 0
                silent = np.setdiff1d(np.arange(n), _flat(ei, es, ns)[:, 0].numpy())
                want = torch.from_numpy(bn)[silent] if with_base else torch.zeros((len(silent), w))
                assert torch.equal(fused[0].cpu()[silent], want)
    print("[mxmnet] edge message W=%d Ka=%d: worst row %.2e of the float32 restatement" % (w, ka, worst))


@pytest.mark.parametrize("w, ka", [(32, 5), (128, 32), (64, 128)])
def test_edge_message_bits(w, ka):
    """Two runs and two streams give equal bits; a shuffled list (the permutation path) gives the bits of the same list
    after a stable reorder by receiver, forward and in the per-edge reverse."""
    ns, es, ei = _edge_list("shuffled")
    n, e = int(ns[-1]), int(es[-1])
    rng = np.random.default_rng(w + ka)
    xn, an = rng.normal(size=(n, w)).astype(np.float32), rng.normal(size=(e, ka)).astype(np.float32)
    bn, gn = rng.normal(size=(n, w)).astype(np.float32), rng.normal(size=(n, w)).astype(np.float32)
    mlp, lin, *_ = _message_layers(w, ka, True, seed=3)
    first = _engine_message("fused", ns, es, ei, xn, an, bn, gn, mlp, lin, "mean")
    again = _engine_message("fused", ns, es, ei, xn, an, bn, gn, mlp, lin, "mean")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = _engine_message("fused", ns, es, ei, xn, an, bn, gn, mlp, lin, "mean")
    side.synchronize()
    for a, b, c in zip(first, again, other):
        assert torch.equal(a, b) and torch.equal(a, c)
    order = np.concatenate([es[g] + np.argsort(ei[es[g]:es[g + 1], 0], kind="stable") for g in range(len(es) - 1)])
    assert not np.array_equal(order, np.arange(e))
    ordered = _engine_message("fused", ns, es, ei[order], xn, an[order], bn, gn, mlp, lin, "mean")
    assert torch.equal(first[0], ordered[0])
    assert torch.equal(first[2][torch.from_numpy(order).to(first[2].device)], ordered[2])
    # the edge epilogue is per edge: rows move with their edges
    ge = rng.normal(size=(e, w)).astype(np.float32)
    y_l = _engine_message("fused", ns, es, ei, xn, an, None, ge, mlp, lin, None)
    y_s = _engine_message("fused", ns, es, ei[order], xn, an[order], None, ge[order], mlp, lin, None)
    dev_order = torch.from_numpy(order).to(y_l[0].device)
    assert torch.equal(y_l[0][dev_order], y_s[0]) and torch.equal(y_l[2][dev_order], y_s[2])


# ------------------------------------------------------------------------------------------------ triplet pool
@functools.lru_cache(maxsize=None)
def _triplet_case(shuffled):
    """Three graphs of 0, 3 and 80 edges.  The second has no triplets; in the third edge 5 receives 70 triplets, edges
    0..9 carry their self pair (n, n), edges from 60 on receive none.  Returns the edge splits, the angle splits and the
    angle list, local to each graph."""
    rng = np.random.default_rng(77)
    es = _splits([0, 3, 80])
    pairs = [[5, int(m)] for m in rng.integers(0, 80, size=70)] + [[n, n] for n in range(10)]
    pairs += [[int(a), int(b)] for a, b in zip(rng.integers(0, 60, size=150), rng.integers(0, 80, size=150))]
    pairs = np.asarray(pairs, dtype=np.int64)
    pairs = pairs[np.argsort(pairs[:, 0], kind="stable")]
    if shuffled:
        pairs = pairs[rng.permutation(len(pairs))]
    return es, _splits([0, 0, len(pairs)]), pairs


def _engine_triplet(layer, fused, es, ts, pairs, xn, sn, gn):
    layer.use_fused_triplet = fused
    x, s, idx = _rag(xn, es), _rag(sn, ts), _rag(pairs, ts)
    xv, sv = x.values.clone().requires_grad_(True), s.values.clone().requires_grad_(True)
    with torch.enable_grad():
        out = layer.triplet_step(x.with_values(xv), s.with_values(sv), idx, layer.gather_mkj, layer.pool_mkj).values
        loss = (out * torch.from_numpy(gn).to(out.device)).sum()
    grads = torch.autograd.grad(loss, [xv, sv], allow_unused=True)
    return [out.detach()] + [torch.zeros_like(t) if g is None else g for t, g in zip((xv, sv), grads)]


def _reference_triplet(dtype, es, ts, pairs, xn, sn, gn, method):
    x = torch.tensor(xn, dtype=dtype, requires_grad=True)
    s = torch.tensor(sn, dtype=dtype, requires_grad=True)
    out = ref.triplet_pool(x, s, _flat(pairs, ts, es), method)
    grads = torch.autograd.grad((out * torch.tensor(gn, dtype=dtype)).sum(), [x, s], allow_unused=True)
    return [out.detach()] + [torch.zeros_like(t) if g is None else g for t, g in zip((x, s), grads)]


def _local_layer(w, method, kr=8, ks=8):
    layer = MXMLocalMP(units=w, pooling_method=method, output_kernel_initializer="glorot_uniform")
    pair = (None, None, 2)
    return layer.ensure_built([(None, None, w), (None, None, kr), (None, None, ks), (None, None, ks), pair, pair, pair])


@pytest.mark.parametrize("method", ["sum", "mean"])
@pytest.mark.parametrize("w", [32, 48])
def test_triplet_pool_fused_sequence_restatement(w, method):
    layer = _local_layer(w, method)
    assert layer.fused_triplet
    for shuffled in (False, True):
        es, ts, pairs = _triplet_case(shuffled)
        e, t = int(es[-1]), int(ts[-1])
        rng = np.random.default_rng(w + t)
        xn, sn = rng.normal(size=(e, w)).astype(np.float32), rng.normal(size=(t, w)).astype(np.float32)
        gn = rng.normal(size=(e, w)).astype(np.float32)
        fused = _engine_triplet(layer, True, es, ts, pairs, xn, sn, gn)
        seq = _engine_triplet(layer, False, es, ts, pairs, xn, sn, gn)
        again = _engine_triplet(layer, True, es, ts, pairs, xn, sn, gn)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            other = _engine_triplet(layer, True, es, ts, pairs, xn, sn, gn)
        side.synchronize()
        r32 = _reference_triplet(F32, es, ts, pairs, xn, sn, gn, method)
        r64 = _reference_triplet(F64, es, ts, pairs, xn, sn, gn, method)
        for name, f, s, a, b, a32, a64 in zip(("out", "x_bar", "s_bar"), fused, seq, again, other, r32, r64):
            what = "triplet W=%d %s shuffled=%s %s" % (w, method, shuffled, name)
            _rows(f, a32, a64, "fused " + what)
            _rows(s, a32, a64, "sequence " + what)
            _rows(f, s, a64, "fused against sequence " + what)
            assert torch.equal(f, a) and torch.equal(f, b), what
        out = fused[0].cpu()
        assert not out[3 + 60:].any() and not out[:3].any()            # edges without triplets: zero rows
        assert float(out[3 + 5].abs().max()) > 0
    # no triplets at all
    es, ts = _splits([0, 3, 80]), _splits([0, 0, 0])
    xn = np.random.default_rng(1).normal(size=(83, w)).astype(np.float32)
    gn = np.ones((83, w), np.float32)
    for fused in (True, False):
        got = _engine_triplet(layer, fused, es, ts, np.zeros((0, 2), np.int64), xn, np.zeros((0, w), np.float32), gn)
        assert tuple(got[0].shape) == (83, w) and not got[0].any() and not got[1].any() and tuple(got[2].shape) == (0, w)


# ------------------------------------------------------------------------------------------------ the two layers
def _set_random_weights(layer, seed):
    ws = list(synth.mxmnet_params(layer, seed=seed, dense_scale=1.0).values())
    layer.set_weights(ws)
    return ws


@pytest.mark.parametrize("units, ka, fused", [(32, 16, True), (128, 128, True), (48, 16, False), (32, 129, False)])
def test_global_layer_routes_and_unsupported_sizes(units, ka, fused):
    """``MXMGlobalMP`` on both routes against the restatement; widths the kernel does not serve (W = 48, Ka = 129) take
    the layer sequence on either setting and still match."""
    layer = MXMGlobalMP(units=units).ensure_built([(None, None, units), (None, None, ka), (None, None, 2)])
    assert layer.fused_step is fused
    ws = _set_random_weights(layer, seed=units + ka)
    for kind in ("batch", "shuffled", "star70"):
        ns, es, ei = _edge_list(kind)
        rng = np.random.default_rng(units + len(kind))
        hn = rng.normal(size=(int(ns[-1]), units)).astype(np.float32)
        an = rng.normal(size=(int(es[-1]), ka)).astype(np.float32)
        flat = _flat(ei, es, ns)
        r32 = ref.global_mp(layer, ws, torch.tensor(hn), torch.tensor(an), flat, F32)
        r64 = ref.global_mp(layer, ws, torch.tensor(hn, dtype=F64), torch.tensor(an, dtype=F64), flat, F64)
        outs = {}
        for on in (True, False):
            layer.use_fused_step = on
            before = _launches()
            with torch.no_grad():
                outs[on] = layer([_rag(hn, ns), _rag(an, es), _rag(ei, es)]).values
            outs[on, "calls"] = _launches() - before
            _rows(outs[on], r32, r64, "MXMGlobalMP units=%d Ka=%d %s fused=%s" % (units, ka, kind, on))
        if fused:
            assert outs[True, "calls"] < outs[False, "calls"]
        else:
            assert outs[True, "calls"] == outs[False, "calls"] and torch.equal(outs[True], outs[False])


def _launches():
    from gcnn_keras_amd import _ffi
    return _ffi.launch_count()


@contextlib.contextmanager
def _engine_calls():
    """The names of the engine calls issued inside, in order."""
    from gcnn_keras_amd import _ffi
    names, real = [], _ffi.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    _ffi.call = call
    try:
        yield names
    finally:
        _ffi.call = real


@pytest.mark.parametrize("units, method", [(32, "sum"), (64, "mean")])
def test_local_layer_routes(units, method):
    """``MXMLocalMP`` (two fused edge messages, two triplet pools, the shared ``h_mlp``) on both routes against the
    restatement, outputs and the gradients of every input."""
    b = ref.model_batch("md17", synth)
    ns, es, s1, s2 = b["node_splits"], b["edge_splits"], b["angle_splits_1"], b["angle_splits_2"]
    kr, ks = 16, 12
    layer = _local_layer(units, method, kr, ks)
    assert layer.fused_step and layer.fused_triplet and layer.use_fused_triplet and not layer.use_fused_step
    ws = _set_random_weights(layer, seed=units)
    rng = np.random.default_rng(units)
    arrays = [rng.normal(size=(int(ns[-1]), units)), rng.normal(size=(int(es[-1]), kr)),
              rng.normal(size=(int(s1[-1]), ks)), rng.normal(size=(int(s2[-1]), ks))]
    arrays = [0.5 * a.astype(np.float32) for a in arrays]
    gh, gy = rng.normal(size=(int(ns[-1]), units)).astype(np.float32), rng.normal(size=(int(ns[-1]), 1)).astype(np.float32)
    ei, ri, a1, a2 = (torch.from_numpy(x) for x in ref.flat_indices(b))

    def restatement(dtype):
        leaves = [torch.tensor(a, dtype=dtype, requires_grad=True) for a in arrays]
        h, y = ref.local_mp(layer, ws, *leaves, ei, a1, a2, dtype=dtype)
        loss = (h * torch.tensor(gh, dtype=dtype)).sum() + (y * torch.tensor(gy, dtype=dtype)).sum()
        return [h.detach(), y.detach()] + list(torch.autograd.grad(loss, leaves))

    def engine(on):
        layer.use_fused_step = layer.use_fused_triplet = on
        rags = [_rag(a, s) for a, s in zip(arrays, (ns, es, s1, s2))]
        leaves = [r.values.clone().requires_grad_(True) for r in rags]
        rags = [r.with_values(v) for r, v in zip(rags, leaves)]
        with torch.enable_grad():
            h, y = layer(rags + [_rag(b["edge_indices"], es), _rag(b["angle_indices_1"], s1),
                                 _rag(b["angle_indices_2"], s2)])
            loss = (h.values * torch.from_numpy(gh).to(h.values.device)).sum() + \
                (y.values * torch.from_numpy(gy).to(h.values.device)).sum()
        return [h.values.detach(), y.values.detach()] + list(torch.autograd.grad(loss, leaves))

    r32, r64 = restatement(F32), restatement(F64)
    fused, seq = engine(True), engine(False)
    for name, f, s, a32, a64 in zip(("h", "y", "h_bar", "rbf_bar", "sbf1_bar", "sbf2_bar"), fused, seq, r32, r64):
        what = "MXMLocalMP units=%d %s %s" % (units, method, name)
        _rows(f, a32, a64, "fused " + what)
        _rows(s, a32, a64, "sequence " + what)
        _rows(f, s, a64, "fused against sequence " + what)


# ------------------------------------------------------------------------------------------------ whole model
def _inputs(b):
    return [_rag(b["node_number"], b["node_splits"]), _rag(b["node_coordinates"], b["node_splits"]),
            _rag(b["edge_weights"], b["edge_splits"]), _rag(b["edge_indices"], b["edge_splits"]),
            _rag(b["angle_indices_1"], b["angle_splits_1"]), _rag(b["angle_indices_2"], b["angle_splits_2"]),
            _rag(b["range_indices"], b["range_splits"])]


@functools.lru_cache(maxsize=None)
def _case(which):
    """The batch, the weights and the restatement's energies and forces of one model case, computed once."""
    b = ref.model_batch(which, synth)
    if which == "default":   # model_default embeds its edge input: integer-valued attributes
        b["edge_weights"] = np.zeros(len(b["edge_indices"]), np.float32)
    cfg = ref.model_config(which, synth, MXMNet)
    m = MXMNet.make_model(**cfg)
    p = list(synth.mxmnet_params(m, seed=ref.WEIGHT_SEED).values())
    return b, cfg, p, ref.energy_forces(p, b, m, F32), ref.energy_forces(p, b, m, F64)


def _model(which):
    b, cfg, p, _, _ = _case(which)
    m = MXMNet.make_model(**cfg)
    m.set_weights(p)
    return m


@pytest.mark.parametrize("which", ["default", "md17"])
def test_model_forward_routes_replay_and_forces(which):
    b, cfg, p, (e32, f32), (e64, f64) = _case(which)
    m = _model(which)
    width = 32 if which == "default" else 128
    assert all(g.fused_step and g.dim == width for g in m.global_blocks)
    assert all(lay.fused_step and lay.fused_triplet for lay in m.local_blocks)
    x = _inputs(b)
    depth = len(m.global_blocks)

    def named(setting):
        """One eager forward under ``model.use_fused_step = setting`` and the names of its engine calls."""
        m.use_fused_step = setting
        with _engine_calls() as names:
            out = m(x)
        assert m.last_route == "eager"
        return out, names

    with torch.no_grad():
        # the routes as they ship: both propagates of every global block and both triplet pools of every
        # local block on their kernels, the local per-edge messages on the layer sequence
        assert m.shipped_routes and not m.use_fused_step
        shipped, names = named(None)
        assert names.count("mp_mxm_edge_f32") == 2 * depth and names.count("mp_mxm_triplet_f32") == 2 * depth, names
        # every fused step on: two more edge messages per local block, no gather and no concatenation left in a block
        first, names = named(True)
        assert m.use_fused_step and not m.shipped_routes
        assert names.count("mp_mxm_edge_f32") == 4 * depth and names.count("mp_mxm_triplet_f32") == 2 * depth, names
        assert "mp_copy_cols_f32" not in names, names               # the concatenation's column copies
        second, third = m(x), m(x)
        assert m.last_route == "graph"                               # a replayed HIP graph: equal bits to eager
        assert torch.equal(first, second) and torch.equal(first, third)
        plain, names = named(False)
        assert not m.use_fused_step and not any(n.startswith("mp_mxm") for n in names), names
        assert "mp_gather_rows_f32" in names and "mp_copy_cols_f32" in names
        m.use_fused_step = None
        assert m.shipped_routes
    assert first.shape == (len(ref.MODEL_SIZES), 1)
    got, off = first.cpu().numpy(), plain.cpu().numpy()
    assert_rows_close(shipped.cpu().numpy(), e32.numpy(), e64.numpy(), what="MXMNet %s forward, default routes" % which)
    assert_rows_close(got, e32.numpy(), e64.numpy(), what="MXMNet %s forward" % which)
    assert_rows_close(off, e32.numpy(), e64.numpy(), what="MXMNet %s forward, layer sequence" % which)
    assert_rows_close(got, off, e64.numpy(), what="MXMNet %s fused against layer sequence" % which)
    # forces of every molecule through EnergyForceModel: the shipped mix, every fused step, the layer sequence
    efm = EnergyForceModel(model_energy=m, coordinate_input=1, output_to_tensor=False, output_squeeze_states=True)
    for on in (None, True, False):
        m.use_fused_step = on
        with _engine_calls() as names:
            eng, force = efm(_inputs(b))
        edge, trip = (0, 0) if on is False else ((4 if on else 2) * depth, 2 * depth)
        assert names.count("mp_mxm_edge_f32") == names.count("mp_mxm_edge_grad_f32") == edge, names
        assert names.count("mp_mxm_triplet_f32") == names.count("mp_mxm_triplet_grad_f32") == trip, names
        assert_rows_close(eng.cpu().numpy().reshape(-1, 1), e32.numpy(), e64.numpy(),
                          what="MXMNet %s EnergyForceModel energy fused=%s" % (which, on))
        assert_forces_close(force.values.cpu().numpy(), f32.numpy(), f64.numpy(), b["node_splits"],
                            what="MXMNet %s forces fused=%s" % (which, on))
        again = efm(_inputs(b))[1].values
        assert torch.equal(force.values, again)


def test_node_embedding_branch_and_edge_attributes():
    b, _, _, _, _ = _case("md17")
    cfg = dict(ref.model_config("md17", synth, MXMNet), output_embedding="node", use_output_mlp=True,
               output_to_tensor=False)
    m = MXMNet.make_model(**cfg)
    p = list(synth.mxmnet_params(m, seed=5).values())
    m.set_weights(p)
    with torch.no_grad():
        got = m(_inputs(b))
    r32, r64 = (ref.mxmnet_forward(p, b, m, dtype=dt) for dt in (F32, F64))
    assert tuple(got.values.shape) == (int(b["node_splits"][-1]), 1)
    _rows(got.values, r32, r64, "MXMNet node branch")
    cfg = dict(ref.model_config("md17", synth, MXMNet), use_edge_attributes=True, depth=1)
    m = MXMNet.make_model(**cfg)
    p = list(synth.mxmnet_params(m, seed=6).values())
    m.set_weights(p)
    with torch.no_grad():
        got = m(_inputs(b))
    r32, r64 = (ref.mxmnet_forward(p, b, m, dtype=dt) for dt in (F32, F64))
    _rows(got, r32, r64, "MXMNet with edge attributes")


def test_train_on_batch_raises_and_leaves_the_weights_untouched():
    b, _, p, _, _ = _case("default")
    m = _model("default")
    m.compile(optimizer="sgd", loss="mean_squared_error")
    with pytest.raises(NotImplementedError):
        m.train_on_batch(_inputs(b), np.zeros((len(ref.MODEL_SIZES), 1), np.float32))
    assert not any(t.requires_grad for t in m.trainable_weights)
    assert all(np.array_equal(a, c) for a, c in zip(p, m.get_weights()))
    efm = EnergyForceModel(model_energy=m, coordinate_input=1, output_to_tensor=False, output_squeeze_states=True)
    efm.compile(optimizer="sgd", loss=["mean_squared_error", "mean_squared_error"])
    with pytest.raises(NotImplementedError):
        efm.train_on_batch(_inputs(b), [np.zeros((len(ref.MODEL_SIZES), 1), np.float32),
                                        np.zeros((int(b["node_splits"][-1]), 3), np.float32)])
    assert all(np.array_equal(a, c) for a, c in zip(p, m.get_weights()))
