"""CGCNN on the engine (csrc/mp_cgcnn.hip, csrc/mp_lattice.hip): the geometry layers, inference batch normalisation, the
fused gate step against the layer sequence and against the torch restatement (tests/cgcnn_reference.py, float32 with the
float64 twin as budget) on graphs that put receivers inside, across and over whole tiles of 32 edges, the whole model
(eager, replayed, ``predict``), training without batch normalisation and the guards."""
import os

import numpy as np
import pytest
import torch

import cgcnn_reference as ref
import periodic_reference as pr
from gcnn_keras_amd import _ffi, synth
from gcnn_keras_amd.layers.conv.cgcnn_conv import CGCNNLayer
from gcnn_keras_amd.layers.geom import DisplacementVectorsUnitCell, FracToRealCoordinates
from gcnn_keras_amd.layers.norm import GraphBatchNormalization
from gcnn_keras_amd.literature import CGCNN
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


def crystal_batch(names, shuffle_seed=None):
    """Golden structures (``"empty"``: a structure without atoms) as one CGCNN batch; ``shuffle_seed``: every structure's
    edge list reordered."""
    numbers, xyz, lats, idx, img, n_sizes, e_sizes = [], [], [], [], [], [], []
    rng = None if shuffle_seed is None else np.random.default_rng(shuffle_seed)
    for k, name in enumerate(names):
        if name == "empty":
            x, lat, i, m = np.zeros((0, 3), np.float32), np.eye(3, dtype=np.float32), np.zeros((0, 2), np.int64), \
                np.zeros((0, 3), np.int64)
        else:
            c = cases()[name]
            x, lat, i, m = c["xyz"], c["lattice"], c["indices"], c["images"]
        if rng is not None:
            order = rng.permutation(len(i))
            i, m = i[order], m[order]
        numbers.append(np.resize(np.array([1, 6, 7, 8, 14], np.int64), len(x)) + k % 3)
        xyz.append(x), lats.append(lat), idx.append(i), img.append(m)
        n_sizes.append(len(x)), e_sizes.append(len(i))
    splits = lambda s: np.concatenate([[0], np.cumsum(s)]).astype(np.int64)
    s = {"node_number": np.concatenate(numbers), "node_coordinates": np.concatenate(xyz, axis=0).astype(np.float32),
         "node_splits": splits(n_sizes), "graph_lattice": np.stack(lats).astype(np.float32)}
    return synth.cgcnn_batch(s, edges={"edge_indices": np.concatenate(idx, axis=0), "edge_image": np.concatenate(img, axis=0),
                                       "edge_splits": splits(e_sizes)})


def model_inputs(b, variant="unit", frac_dtype=np.float32):
    x = [_rag(b["node_number"], b["node_splits"]),
         _rag(b["node_frac_coordinates"].astype(frac_dtype), b["node_splits"]),
         _rag(b["edge_indices"], b["edge_splits"]),
         torch.from_numpy(b["lattice_matrix"].astype(frac_dtype)).cuda()]
    if variant == "unit":
        x.append(_rag(b["cell_translations"], b["edge_splits"]))
    return x


# ------------------------------------------------------------------------------------------------ geometry
def _frac_to_real_np(f, lat_rows):
    """float32, the kernel's stated order: r_k = (f_0 A[k][0] + f_1 A[k][1]) + f_2 A[k][2]."""
    f, a = np.asarray(f, np.float32), np.asarray(lat_rows, np.float32)
    return np.stack([(f[:, 0] * a[:, k, 0] + f[:, 1] * a[:, k, 1]) + f[:, 2] * a[:, k, 2] for k in range(3)], axis=1)


def _frac_to_real_t_np(g, lat_rows):
    g, a = np.asarray(g, np.float32), np.asarray(lat_rows, np.float32)
    return np.stack([(g[:, 0] * a[:, 0, j] + g[:, 1] * a[:, 1, j]) + g[:, 2] * a[:, 2, j] for j in range(3)], axis=1)


def test_frac_to_real_is_bit_exact_and_linear():
    rng = np.random.default_rng(1)
    sizes = [5, 0, 1, 300, 0]
    splits = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    f = rng.normal(size=(splits[-1], 3)).astype(np.float32)
    lat = rng.normal(size=(len(sizes), 3, 3)).astype(np.float32) * 4
    rows = np.repeat(lat, sizes, axis=0)
    layer = FracToRealCoordinates()
    lat_d = torch.from_numpy(lat).cuda()
    with torch.no_grad():
        out = layer([_rag(f, splits), lat_d]).values
    want = _frac_to_real_np(f, rows)
    assert np.array_equal(out.cpu().numpy(), want)
    # A f, not f A: the einsum as written
    np.testing.assert_allclose(want, np.einsum("ij,ikj->ik", f.astype(np.float64), rows.astype(np.float64)), rtol=0,
                               atol=1e-4)
    # the reverse is the transposed product, and it is differentiable again (linear)
    fv = torch.from_numpy(f).cuda().requires_grad_(True)
    g = torch.from_numpy(rng.normal(size=f.shape).astype(np.float32)).cuda().requires_grad_(True)
    v = torch.from_numpy(rng.normal(size=f.shape).astype(np.float32)).cuda()
    with torch.enable_grad():
        y = layer([_rag(f, splits).with_values(fv), lat_d]).values
        (f_bar,) = torch.autograd.grad(y, [fv], g, create_graph=True)
        (g_bar,) = torch.autograd.grad(f_bar, [g], v)
    assert torch.equal(y.detach(), out)
    assert np.array_equal(f_bar.detach().cpu().numpy(), _frac_to_real_t_np(g.detach().cpu().numpy(), rows))
    assert np.array_equal(g_bar.cpu().numpy(), _frac_to_real_np(v.cpu().numpy(), rows))
    with torch.enable_grad(), pytest.raises(NotImplementedError, match="lattice"):
        layer([_rag(f, splits), lat_d.clone().requires_grad_(True)])
    with pytest.raises(ValueError):
        layer([_rag(f, splits), lat_d[:3]])
    assert _ffi.lib().mp_frac_to_real_f32(None, None, None, 0, 0, 0, None, None) == _ffi.MP_OK
    assert _ffi.lib().mp_frac_to_real_f32(None, None, None, 1, 4, 0, None, None) == _ffi.MP_EINVAL


def test_displacement_unit_cell_and_golden_distances():
    b = crystal_batch(["tri5_c40", "empty", "thin2_c40"])
    frac, ei = _rag(b["node_frac_coordinates"], b["node_splits"]), _rag(b["edge_indices"], b["edge_splits"])
    flat = ref.flat_edges(b)
    f = b["node_frac_coordinates"]
    want = f[flat[:, 0]] - (f[flat[:, 1]] + b["cell_translations"])
    layer = DisplacementVectorsUnitCell()
    with torch.no_grad():
        d32 = layer([frac, ei, _rag(b["cell_translations"], b["edge_splits"])]).values
        d64 = layer([frac, ei, _rag(b["cell_translations"].astype(np.int64), b["edge_splits"])]).values   # range_image
        real = FracToRealCoordinates()([ei.with_values(d32), torch.from_numpy(b["lattice_matrix"]).cuda()]).values
    assert np.array_equal(d32.cpu().numpy(), want) and torch.equal(d32, d64)
    dist = np.linalg.norm(real.cpu().numpy().astype(np.float64), axis=1)
    golden = np.concatenate([cases()["tri5_c40"]["dist"], cases()["thin2_c40"]["dist"]])
    # float32 fractional coordinates of magnitude <= 4 against cells of ~6 A: a few ulp of 6 A
    assert np.max(np.abs(dist - golden)) <= 2e-5
    fv = frac.values.clone().requires_grad_(True)
    with torch.enable_grad():
        out = layer([frac.with_values(fv), ei, _rag(b["cell_translations"], b["edge_splits"])]).values
        (f_bar,) = torch.autograd.grad(out.sum(), [fv])
    deg = np.bincount(flat[:, 0], minlength=len(f)) - np.bincount(flat[:, 1], minlength=len(f))
    np.testing.assert_allclose(f_bar.cpu().numpy(), np.repeat(deg[:, None], 3, axis=1).astype(np.float32), atol=1e-4)


# ------------------------------------------------------------------------------------------------ batch normalisation
def _bn_vectors(rng, width):
    return [rng.uniform(0.5, 1.5, width), rng.uniform(-0.3, 0.3, width), rng.uniform(-0.5, 0.5, width),
            rng.uniform(0.5, 2.0, width)]


@pytest.mark.parametrize("scale,center", [(True, True), (False, True), (True, False)])
def test_batch_norm_inference_forward_and_input_gradient(scale, center):
    rng = np.random.default_rng(2)
    rows, width = 77, 64
    x = rng.normal(size=(rows, width)).astype(np.float32)
    g = rng.normal(size=(rows, width)).astype(np.float32)
    layer = GraphBatchNormalization(scale=scale, center=center, epsilon=1e-3).ensure_built((None, None, width))
    vec = [v.astype(np.float32) for v in _bn_vectors(rng, width)]
    layer.set_weights([v for v, on in zip(vec, (scale, center, True, True)) if on])
    splits = np.array([0, 30, 30, rows])
    xv = torch.from_numpy(x).cuda().requires_grad_(True)
    with torch.enable_grad():
        y = layer(_rag(x, splits).with_values(xv)).values
        (x_bar,) = torch.autograd.grad(y, [xv], torch.from_numpy(g).cuda())
    with torch.no_grad():
        plain = layer(_rag(x, splits)).values
    assert torch.equal(plain, y.detach())
    outs = {}
    for dt in (np.float32, np.float64):
        gamma = vec[0].astype(dt) if scale else np.ones(width, dt)
        beta = vec[1].astype(dt) if center else np.zeros(width, dt)
        inv = (dt(1) / np.sqrt(vec[3].astype(dt) + dt(1e-3))) * gamma
        outs[dt] = (x.astype(dt) * inv + (beta - vec[2].astype(dt) * inv), g.astype(dt) * inv)
    assert_rows_close(y.detach().cpu().numpy(), outs[np.float32][0], outs[np.float64][0], what="batch norm forward")
    assert_rows_close(x_bar.cpu().numpy(), outs[np.float32][1], outs[np.float64][1], what="batch norm input gradient")
    # the vectors are read in place: new statistics are seen by the next call
    layer.moving_mean.add_(1.0)
    with torch.no_grad():
        assert not torch.equal(layer(_rag(x, splits)).values, plain)


def test_batch_norm_guards():
    layer = GraphBatchNormalization().ensure_built((None, None, 8))
    x = _rag(np.zeros((3, 8), np.float32), np.array([0, 3]))
    with pytest.raises(NotImplementedError, match="training"):
        layer(x, training=True)
    with pytest.raises(NotImplementedError):
        GraphBatchNormalization(axis=1)(_rag(np.zeros((3, 8, 2), np.float32), np.array([0, 3])))
    layer.gamma.requires_grad_(True)
    try:
        with torch.enable_grad(), pytest.raises(NotImplementedError, match="weight gradients"):
            layer(x)
    finally:
        layer.gamma.requires_grad_(False)
    lib = _ffi.lib()
    assert lib.mp_batchnorm_infer_f32(None, 0, 8, None, None, None, None, 1e-3, None, None) == _ffi.MP_OK
    assert lib.mp_batchnorm_infer_f32(None, 4, 8, None, None, None, None, 1e-3, None, None) == _ffi.MP_EINVAL


# ------------------------------------------------------------------------------------------------ fused gate step
CONFIGS = {
    "plain": dict(batch_normalization=False),
    "bn": dict(batch_normalization=True),
    "bn_nobias_swish_linear": dict(batch_normalization=True, use_bias=False, activation_s="swish",
                                   activation_out="linear"),
    "nobias_swish_linear": dict(batch_normalization=False, use_bias=False, activation_s="swish", activation_out="linear"),
}


def _edge_features(dist, width):
    """(E, width) float32 edge features of distances (E,): the distance itself, or a Gauss basis of ``width`` bins."""
    d = torch.from_numpy(np.asarray(dist, np.float32).reshape(-1, 1))
    if width == 1:
        return d.numpy()
    return ref.gauss_basis(d, {"bins": width, "distance": 8, "sigma": 0.4, "offset": 0.0}, torch.float32).numpy()


def graph_case(name, width=40, seed=0):
    """``(h (N, 64), features (E, width), edge_indices, node_splits, edge_splits)`` of a named layer-level case."""
    rng = np.random.default_rng(seed)
    if name.startswith("hand"):
        # 4 nodes, node 2 without edges, receivers sorted, any sender
        e = int(name[4:])
        recv = np.sort(rng.choice(np.array([0, 1, 3]), size=e))
        idx = np.stack([recv, rng.integers(0, 4, size=e)], axis=1).astype(np.int64).reshape(-1, 2)
        b = {"edge_indices": idx, "node_splits": np.array([0, 4]), "edge_splits": np.array([0, e])}
        dist = rng.uniform(0.8, 6.0, size=e)
    else:
        names = {"batch": ["tri5_c40", "empty", "cubic1_c40", "big6_c40", "empty"],
                 "batch_shuffled": ["tri5_c40", "empty", "cubic1_c40", "big6_c40", "empty"]}.get(name, [name])
        b = crystal_batch(names, shuffle_seed=4 if name == "batch_shuffled" else None)
        dist = ref.edge_distances(b, {"representation": "unit"}, torch.float64).numpy().reshape(-1)
    n = int(b["node_splits"][-1])
    h = rng.normal(size=(n, 64)).astype(np.float32)
    return h, _edge_features(dist, width), b["edge_indices"], b["node_splits"], b["edge_splits"]


def make_layer(width, seed, **kwargs):
    rng = np.random.default_rng(seed)
    lay = CGCNNLayer(**kwargs)
    lay.ensure_built([(None, None, 64), (None, None, width), (None, None, 2)])
    ws = []
    for name, t in lay.weights:
        leaf, shape = name.rsplit("/", 1)[-1], tuple(t.shape)
        if leaf == "kernel":
            ws.append(synth.glorot_uniform(rng, shape[0], shape[1], shape=shape))
        elif leaf == "bias":
            ws.append(rng.uniform(-0.1, 0.1, shape))
        else:
            ws.append(dict(zip(("gamma", "beta", "moving_mean", "moving_variance"), _bn_vectors(rng, 64)))[leaf])
    lay.set_weights([np.asarray(w, np.float32) for w in ws])
    return lay


def _ref_layer(lay, h, feats, flat, dtype):
    it = iter([torch.tensor(w, dtype=dtype) for w in lay.get_weights()])
    w = ref.take_layer_weights(it, lay.batch_normalization, lay.use_bias)
    _, out = ref.cgcnn_layer(torch.tensor(h, dtype=dtype), torch.tensor(feats, dtype=dtype), torch.from_numpy(flat), w,
                             lay.activation_s_layer.activation, lay.activation_out_layer.activation)
    return out.numpy(), w


def check_gate_case(name, width, config, seed=0):
    h, feats, idx, ns, es = graph_case(name, width, seed)
    lay = make_layer(width, seed + 1, **CONFIGS[config])
    assert lay.fused_gate is True
    x = [_rag(h, ns), _rag(feats, es), _rag(idx, es)]
    launches = _ffi.launch_count()
    with torch.no_grad():
        fused = lay(x).values
        fused_launches = _ffi.launch_count() - launches
        again = lay(x).values
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            other = lay(x).values
        s.synchronize()
        lay.use_fused_gate = False
        launches = _ffi.launch_count()
        seq = lay(x).values
        seq_launches = _ffi.launch_count() - launches
        lay.use_fused_gate = True
    assert torch.equal(fused, again) and torch.equal(fused, other)
    assert fused_launches < seq_launches                      # the fused kernel ran, not the layer sequence
    flat = ref.flat_edges({"edge_indices": idx, "node_splits": ns, "edge_splits": es})
    r32, _ = _ref_layer(lay, h, feats, flat, torch.float32)
    r64, w64 = _ref_layer(lay, h, feats, flat, torch.float64)
    what = "gate step %s D=%d %s" % (name, width, config)
    got, other = fused.cpu().numpy(), seq.cpu().numpy()
    assert got.shape == r64.shape == (len(h), 64)
    assert_rows_close(got, r32, r64, what=what)
    assert_rows_close(other, r32, r64, what=what + " (layer sequence)")
    bar = max(1e-5, min(2 * rowwise_rel(r32, r64), 5e-5))
    assert rowwise_rel(got, other) <= 2 * bar, "%s: fused vs layer sequence %.3g" % (what, rowwise_rel(got, other))
    # nodes without edges: u = 0, and BN_out(0) = beta - mean * inv is not zero
    lone = np.bincount(flat[:, 0], minlength=len(h)) == 0
    if lone.any():
        shift = 0.0
        if lay.batch_normalization:
            gamma, beta, mean, var = [t.numpy() for t in w64["bn_out"]]
            inv = gamma / np.sqrt(var + ref.BN_EPSILON)
            shift = beta - mean * inv
            assert np.min(np.abs(shift)) > 0
        want = ref.ACTIVATIONS[lay.activation_out_layer.activation](torch.tensor(h[lone].astype(np.float64) + shift))
        assert_rows_close(got[lone], want.numpy().astype(np.float32), want.numpy(), what=what + " isolated nodes")
    return lone


GRAPHS = ["big6_c40", "cubic1_c40", "thin2_c40", "tri5_c40_n12", "tri5_c40", "tri5_c55", "hand0", "hand1", "hand31",
          "hand32", "hand33", "hand64", "hand65", "batch", "batch_shuffled"]


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("name", GRAPHS)
def test_fused_gate_step_graphs(name, config):
    lone = check_gate_case(name, 40, config)
    if name in ("big6_c40", "batch") or name.startswith("hand"):
        assert lone.any()


@pytest.mark.parametrize("config", ["plain", "bn_nobias_swish_linear"])
@pytest.mark.parametrize("width", [1, 41, 64])
@pytest.mark.parametrize("name", ["tri5_c40", "batch_shuffled", "hand33"])
def test_fused_gate_step_edge_widths(name, width, config):
    check_gate_case(name, width, config, seed=3)


def test_graph_cases_cut_receivers_as_the_issue_says():
    deg = lambda n: np.bincount(cases()[n]["indices"][:, 0], minlength=len(cases()[n]["xyz"]))
    assert len(cases()["thin2_c40"]["indices"]) == 42 and deg("thin2_c40")[0] < 32 < deg("thin2_c40").sum()
    assert deg("tri5_c40").min() >= 45 and deg("tri5_c55").min() >= 124       # every receiver cut / whole middle tiles
    assert np.sum(deg("big6_c40") == 0) >= 2 and len(cases()["cubic1_c40"]["xyz"]) == 1
    starts = np.concatenate([[0], np.cumsum(deg("tri5_c55"))])
    assert any((-(-a // 32) + 1) * 32 <= b for a, b in zip(starts[:-1], starts[1:]))   # a receiver owns a whole tile


def test_fused_gate_step_guards():
    h, feats, idx, ns, es = graph_case("thin2_c40", 40)
    lay = make_layer(40, 1, batch_normalization=True)
    x = [_rag(h, ns), _rag(feats, es), _rag(idx, es)]
    with torch.no_grad():
        base = lay(x).values
    # any tape takes the layer sequence: an input that requires grad ...
    hv = torch.from_numpy(h).cuda().requires_grad_(True)
    with torch.enable_grad():
        launches = _ffi.launch_count()
        out = lay([x[0].with_values(hv), x[1], x[2]]).values
        assert _ffi.launch_count() - launches > 8
        (h_bar,) = torch.autograd.grad(out.sum(), [hv])
    assert_rows_close(out.detach().cpu().numpy(), base.cpu().numpy(), what="layer sequence on a tape")
    assert float(h_bar.abs().max()) > 0
    # ... or a weight that requires grad: the Dense kernels get their gradients from the existing rules,
    lay.s.kernel.requires_grad_(True)
    try:
        with torch.enable_grad():
            launches = _ffi.launch_count()
            out = lay(x).values
            assert _ffi.launch_count() - launches > 8
            (k_bar,) = torch.autograd.grad(out.sum(), [lay.s.kernel])
        assert float(k_bar.abs().max()) > 0
        with torch.no_grad():
            assert torch.equal(lay(x).values, base)
    finally:
        lay.s.kernel.requires_grad_(False)
    # a batch-norm vector has none and raises instead of training against frozen statistics
    lay.batch_norm_s.gamma.requires_grad_(True)
    try:
        with torch.enable_grad(), pytest.raises(NotImplementedError, match="weight gradients"):
            lay(x)
    finally:
        lay.batch_norm_s.gamma.requires_grad_(False)
    # out-of-range edges raise before the kernel runs
    bad = idx.copy()
    bad[3, 1] = 7
    with pytest.raises(IndexError):
        lay([x[0], x[1], _rag(bad, es)])
    lib = _ffi.lib()
    args = [None] * 5 + [4, None, 40, None, 0] + [None] * 8 + [3, 3, 0.05, None, 0, None, None]
    assert lib.mp_cgcnn_gate_f32(*args) == _ffi.MP_EINVAL                   # null pointers
    args[5] = 0
    assert lib.mp_cgcnn_gate_f32(*args) == _ffi.MP_OK                       # no nodes: nothing to do
    args[7] = 65
    assert lib.mp_cgcnn_gate_f32(*args) == _ffi.MP_EINVAL                   # D > 64
    args[7], args[9] = 40, 2 ** 31
    assert lib.mp_cgcnn_gate_f32(*args) == _ffi.MP_EINVAL                   # E at 2^31


# ------------------------------------------------------------------------------------------------ model
BATCH = ["tri5_c40", "empty", "cubic1_c40", "big6_c40", "empty"]
# predict(batch_size=2) cuts [tri5, cubic1] and [empty, big6]: node pooling drops TRAILING empty graphs of a call (the
# reference's segment ops), so the data set is ordered to end no batch on one
PREDICT_BATCH = ["tri5_c40", "cubic1_c40", "empty", "big6_c40"]


def _model(seed=14, **cfg):
    m = CGCNN.make_crystal_model(**cfg)
    p = list(synth.cgcnn_params(m, seed=seed).values())
    m.set_weights(p)
    return m, p


@pytest.mark.parametrize("shuffled", [False, True])
def test_model_defaults_match_restatement(shuffled):
    b = crystal_batch(BATCH, shuffle_seed=6 if shuffled else None)
    m, p = _model()
    assert m.fused_gate_layers == [True] * 3 and m.config["conv_layer_args"]["batch_normalization"] is True
    x = model_inputs(b)
    with torch.no_grad():
        got = m(x).cpu().numpy()
        m.use_fused_gate = False
        seq = m(x).cpu().numpy()
        m.use_fused_gate = True
    r32 = ref.cgcnn_forward(p, b, m.config, dtype=torch.float32).numpy()
    r64 = ref.cgcnn_forward(p, b, m.config, dtype=torch.float64).numpy()
    assert got.shape == seq.shape == (4, 1) and r64.shape == (5, 1)     # the trailing empty structure is dropped
    assert_rows_close(got, r32[:4], r64[:4], what="CGCNN defaults, fused")
    assert_rows_close(seq, r32[:4], r64[:4], what="CGCNN defaults, layer sequence")


def test_model_eager_replay_predict_and_stale_weights():
    b = crystal_batch(PREDICT_BATCH)
    m, _ = _model()
    x = model_inputs(b)
    with torch.no_grad():
        first = m(x)
        assert m.last_route == "eager"
        second = m(x)
        third = m(x)
        assert m.last_route == "graph"
        served = m.predict(x, batch_size=2)
    assert torch.equal(first, second) and torch.equal(first, third) and torch.equal(first, served)
    assert tuple(first.shape) == (4, 1)
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
    m.use_fused_gate = False
    with torch.no_grad():
        seq = m(x)
    assert m.last_route == "eager"
    m.use_fused_gate = True
    assert_rows_close(seq.cpu().numpy(), eager.cpu().numpy(), what="layer sequence after the switch")
    # the per-layer switch is part of a captured graph's identity too
    m.conv_layers[1].use_fused_gate = False
    with torch.no_grad():
        m(x)
    assert m.last_route == "eager" and m.use_fused_gate is False
    m.conv_layers[1].use_fused_gate = True


def test_model_input_variants_and_float64():
    b = crystal_batch(PREDICT_BATCH)
    m, p = _model()
    with torch.no_grad():
        base = m(model_inputs(b))
        as64 = m(model_inputs(b, frac_dtype=np.float64))
        image = model_inputs(b)
        image[4] = _rag(b["cell_translations"].astype(np.int64), b["edge_splits"])     # SetRangePeriodic's range_image
        from_image = m(image)
    assert torch.equal(base, as64) and torch.equal(base, from_image)
    # four inputs: no cell translations (every edge inside the cell), x_out - x_in
    m4, p4 = _model(representation=None, inputs=CGCNN.model_crystal_default["inputs"][:4])
    with torch.no_grad():
        got = m4(model_inputs(b, variant=None)).cpu().numpy()
    r32 = ref.cgcnn_forward(p4, b, m4.config, dtype=torch.float32).numpy()
    r64 = ref.cgcnn_forward(p4, b, m4.config, dtype=torch.float64).numpy()
    assert_rows_close(got, r32, r64, what="CGCNN four inputs")
    # three inputs: distances given; bare (expand_distance=False) and expanded
    dist = ref.edge_distances(b, {"representation": "unit"}, torch.float64).numpy().astype(np.float32)
    b3 = dict(b, edge_distance=dist)
    inputs3 = [CGCNN.model_crystal_default["inputs"][0],
               {"shape": (None, 1), "name": "edge_distance", "dtype": "float32", "ragged": True},
               CGCNN.model_crystal_default["inputs"][2]]
    for expand in (True, False):
        m3, p3 = _model(make_distances=False, expand_distance=expand, inputs=inputs3)
        assert m3.fused_gate_layers == [True] * 3
        x3 = [_rag(b["node_number"], b["node_splits"]), _rag(dist, b["edge_splits"]),
              _rag(b["edge_indices"], b["edge_splits"])]
        with torch.no_grad():
            got = m3(x3).cpu().numpy()
        r32 = ref.cgcnn_forward(p3, b3, m3.config, dtype=torch.float32).numpy()
        r64 = ref.cgcnn_forward(p3, b3, m3.config, dtype=torch.float64).numpy()
        assert_rows_close(got, r32, r64, what="CGCNN three inputs expand=%s" % expand)


def test_set_range_periodic_output_feeds_the_model():
    from gcnn_keras_amd.graph.preprocessor import SetRangePeriodic
    s = synth.periodic_structures(num_graphs=6, seed=9, max_atoms=9)
    xyz = _rag(s["node_coordinates"], s["node_splits"])
    idx, img, dist = SetRangePeriodic(max_distance=5.0, max_neighbours=12)(xyz, torch.from_numpy(s["graph_lattice"]).cuda())
    b = synth.cgcnn_batch(s, edges={"range_indices": idx.values.cpu().numpy(), "range_image": img.values.cpu().numpy(),
                                    "edge_splits": idx.row_splits.cpu().numpy()})
    assert img.values.dtype == torch.int64 and len(b["edge_indices"]) == 12 * len(s["node_number"])
    m, p = _model()
    x = [_rag(b["node_number"], b["node_splits"]), _rag(b["node_frac_coordinates"], b["node_splits"]), idx,
         torch.from_numpy(b["lattice_matrix"]).cuda(), img]        # range_indices / range_image as they come
    with torch.no_grad():
        got = m(x).cpu().numpy()
    r32 = ref.cgcnn_forward(p, b, m.config, dtype=torch.float32).numpy()
    r64 = ref.cgcnn_forward(p, b, m.config, dtype=torch.float64).numpy()
    assert_rows_close(got, r32, r64, what="CGCNN on SetRangePeriodic output")
    # the model's distances are those of the search: the lattice went in transposed
    d = ref.edge_distances(b, m.config, torch.float64).numpy()
    assert np.max(np.abs(d - dist.values.cpu().numpy())) <= 2e-5


# ------------------------------------------------------------------------------------------------ training
TRAIN_BATCH = ["tri5_c40_n12", "cubic1_c40", "big6_c40", "thin2_c40"]


def test_weight_gradients_match_restatement_autograd():
    b = crystal_batch(TRAIN_BATCH)
    m, p = _model(conv_layer_args={"batch_normalization": False}, depth=2)
    x = model_inputs(b)
    target = np.random.default_rng(4).normal(size=(4, 1)).astype(np.float32)
    m.requires_grad_(True)
    try:
        with torch.enable_grad():
            loss = (m(x) - torch.from_numpy(target).cuda()).abs().mean()
            loss.backward()
        grads = [t.grad.detach().cpu().numpy() for t in m.trainable_weights]
    finally:
        m.requires_grad_(False)
        for t in m.trainable_weights:
            t.grad = None
    refs = {}
    for dt in (torch.float32, torch.float64):
        w = [torch.tensor(a, dtype=dt, requires_grad=True) for a in p]
        rl = (ref.cgcnn_forward(w, b, m.config, dtype=dt) - torch.from_numpy(target).to(dt)).abs().mean()
        refs[dt] = (float(rl.detach()), [g.numpy() for g in torch.autograd.grad(rl, w)])
    np.testing.assert_allclose(float(loss.detach()), refs[torch.float64][0], rtol=1e-5)
    for (name, _), g, g32, g64 in zip(m.weights, grads, refs[torch.float32][1], refs[torch.float64][1]):
        # the bar of the EGNN energy-training test (1e-5 of the tensor's scale), raised to the float32 restatement's own
        # distance from float64 where that is larger (a float32 tape cannot do better), as parity.assert_rows_close does
        scale = max(float(np.max(np.abs(g64))), 1e-3)
        e32 = float(np.max(np.abs(g32 - g64))) / scale
        err = float(np.max(np.abs(g - g64))) / scale
        print("[training] %s: gradient %.2e of its scale from float64 (float32 restatement %.2e)" % (name, err, e32))
        assert err <= max(1e-5, min(4 * e32, 5e-5)), name
        if np.max(np.abs(g64)) > 0:
            assert np.max(np.abs(g)) > 0, name


def test_sgd_trajectory_and_fit_without_batch_norm():
    b = crystal_batch(TRAIN_BATCH)
    m, p = _model(conv_layer_args={"batch_normalization": False}, depth=2)
    x = model_inputs(b)
    target = np.random.default_rng(5).normal(size=(4, 1)).astype(np.float32)
    # outputs of the random model are ~10 (mean pooling of softplus rows through a Glorot MLP): lr 1e-5 keeps the five
    # steps a descent, so the trajectory is not a chaotic one that amplifies float32 rounding
    m.compile(optimizer=torch.optim.SGD(m.trainable_weights, lr=1e-5), loss="mean_absolute_error")
    losses = [m.train_on_batch(x, target) for _ in range(5)]
    assert not any(t.requires_grad for t in m.trainable_weights)
    w = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in p]
    opt = torch.optim.SGD(w, lr=1e-5)
    ref_losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = (ref.cgcnn_forward(w, b, m.config) - torch.from_numpy(target).double()).abs().mean()
        loss.backward()
        opt.step()
        ref_losses.append(float(loss.detach()))
    print("[training] engine %s restatement %s" % (losses, ref_losses))
    np.testing.assert_allclose(losses, ref_losses, rtol=1e-5)
    assert len(set(losses)) == 5
    # the fused route serves the trained weights
    with torch.no_grad():
        after = m(x).cpu().numpy()
    r64 = ref.cgcnn_forward([t.detach() for t in w], b, m.config).numpy()
    r32 = ref.cgcnn_forward([t.detach() for t in w], b, m.config, dtype=torch.float32).numpy()
    assert_rows_close(after, r32, r64, what="trained weights, fused")
    history = m.fit(x, target, batch_size=2, epochs=2, seed=1)
    assert len(history.history["loss"]) == 2 and all(np.isfinite(v) for v in history.history["loss"])


def test_training_a_batch_normalised_model_raises():
    b = crystal_batch(TRAIN_BATCH)
    m, _ = _model(depth=1)
    m.compile(optimizer="sgd", loss="mean_absolute_error")
    before = m.get_weights()
    with pytest.raises(NotImplementedError, match="weight gradients"):
        m.train_on_batch(model_inputs(b), np.zeros((4, 1), np.float32))
    assert not any(t.requires_grad for t in m.trainable_weights)
    assert all(np.array_equal(a, c) for a, c in zip(before, m.get_weights()))
