"""CGCNN without a GPU: configuration keys of the four new layers against the reference's key lists, the builder's
refusals, weight names / shapes / order, the decisions of ``fused_gate_supported``, and the restatement
(tests/cgcnn_reference.py) pinned: against a per-edge NumPy loop, against the golden distances of the periodic cases
(lattice transposed: the reference's einsum is ``A f``) and by the super-cell identity in float64."""
import numpy as np
import pytest
import torch

import cgcnn_reference as ref
import periodic_reference as pr
from gcnn_keras_amd import synth
from gcnn_keras_amd.layers.conv.cgcnn_conv import FUSED_GATE_SIZES, CGCNNLayer, fused_gate_supported
from gcnn_keras_amd.layers.geom import DisplacementVectorsUnitCell, FracToRealCoordinates
from gcnn_keras_amd.layers.norm import GraphBatchNormalization
from gcnn_keras_amd.literature import CGCNN

BASE_KEYS = {"name", "trainable", "dtype", "node_indexing", "ragged_validate", "is_sorted", "has_unconnected"}
# kgcnn/layers/norm.py:180-183 and :221 - the key list misses a comma, so "moving_variance_initializer" and
# "beta_regularizer" fuse into one name that no Keras config holds: neither is part of the reference's get_config()
BATCH_NORM_KEYS = BASE_KEYS | {"axis", "momentum", "epsilon", "scale", "center", "beta_initializer", "gamma_initializer",
                               "moving_mean_initializer", "gamma_regularizer", "beta_constraint", "gamma_constraint"}
# kgcnn/layers/conv/cgcnn_conv.py:113-128 on top of MessagePassingBase (kgcnn/layers/message.py: pooling_method)
CGCNN_LAYER_KEYS = BASE_KEYS | {"pooling_method", "units", "use_bias", "batch_normalization", "activation_s",
                                "activation_out", "activity_regularizer", "kernel_regularizer", "bias_regularizer",
                                "kernel_constraint", "bias_constraint", "kernel_initializer", "bias_initializer"}


@pytest.fixture(scope="module")
def cases(golden_dir):
    return pr.golden_cases(golden_dir)


# ------------------------------------------------------------------------------------------------ configuration
@pytest.mark.parametrize("cls,kwargs,keys", [
    (DisplacementVectorsUnitCell, {}, BASE_KEYS),
    (FracToRealCoordinates, {}, BASE_KEYS),
    (GraphBatchNormalization, {"epsilon": 0.01, "momentum": 0.9, "center": False}, BATCH_NORM_KEYS),
    (CGCNNLayer, {"units": 32, "activation_s": "swish", "activation_out": "linear", "batch_normalization": True,
                  "use_bias": False}, CGCNN_LAYER_KEYS),
], ids=["displacement", "frac_to_real", "batch_norm", "cgcnn_layer"])
def test_config_keys_and_round_trip(cls, kwargs, keys):
    layer = cls(**kwargs)
    config = layer.get_config()
    assert set(config) == keys
    for k, v in kwargs.items():
        assert config[k] == v
    again = cls.from_config(config)
    assert again.get_config() == config


def test_batch_norm_axis_and_training_guards():
    with pytest.raises(ValueError):
        GraphBatchNormalization(axis=0)
    with pytest.raises(TypeError):
        GraphBatchNormalization(axis="last")
    with pytest.raises(NotImplementedError):
        GraphBatchNormalization(axis=1).ensure_built((None, None, 8))      # not the last axis
    layer = GraphBatchNormalization(axis=2).ensure_built((None, None, 8))
    assert layer.axis == 2 and [n for n, _ in layer.weights] == ["gamma", "beta", "moving_mean", "moving_variance"]
    assert np.all(layer.get_weights()[0] == 1) and np.all(layer.get_weights()[3] == 1)
    assert np.all(layer.get_weights()[1] == 0) and np.all(layer.get_weights()[2] == 0)
    bare = GraphBatchNormalization(scale=False, center=False).ensure_built((None, None, 8))
    assert [n for n, _ in bare.weights] == ["moving_mean", "moving_variance"]
    assert GraphBatchNormalization.weight_gradients is False
    with pytest.raises(NotImplementedError):
        layer(torch.zeros(3, 8), training=True)


# ------------------------------------------------------------------------------------------------ builder
def test_builder_defaults_and_refusals():
    d = CGCNN.model_crystal_default
    assert [i["name"] for i in d["inputs"]] == ["node_number", "node_frac_coordinates", "edge_indices", "lattice_matrix",
                                                "cell_translations"]
    assert d["representation"] == "unit" and d["expand_distance"] and d["make_distances"] and d["depth"] == 3
    assert d["gauss_args"] == {"bins": 40, "distance": 8, "offset": 0.0, "sigma": 0.4}
    assert d["conv_layer_args"] == {"units": 64, "activation_s": "softplus", "activation_out": "softplus",
                                    "batch_normalization": True}
    assert d["node_pooling_args"] == {"pooling_method": "mean"} and d["input_embedding"] == {
        "node": {"input_dim": 95, "output_dim": 64}}
    assert d["output_mlp"] == {"use_bias": [True, False], "units": [64, 1], "activation": ["softplus", "linear"]}
    with pytest.raises(NotImplementedError, match="asu"):
        CGCNN.make_crystal_model(representation="asu")
    with pytest.raises(ValueError, match="Unsupported output embedding"):
        CGCNN.make_crystal_model(output_embedding="node")
    with pytest.raises(ValueError):
        CGCNN.make_crystal_model(no_such_key=1)
    assert "transposed" in CGCNN.make_crystal_model.__doc__ and "transposed" in FracToRealCoordinates.__doc__.lower()


@pytest.mark.parametrize("batch_norm", [True, False])
def test_weight_names_shapes_and_order(batch_norm):
    m = CGCNN.make_crystal_model(depth=2, conv_layer_args={"batch_normalization": batch_norm})
    leaves = [(n.rsplit("/", 1)[-1], tuple(t.shape)) for n, t in m.weights]
    bn = [(v, (64,)) for v in ("gamma", "beta", "moving_mean", "moving_variance")] * 3 if batch_norm else []
    layer = bn + [("kernel", (168, 64)), ("bias", (64,))] * 2
    want = [("embeddings", (95, 64)), ("kernel", (64, 64)), ("bias", (64,))] + layer * 2 + [
        ("kernel", (64, 64)), ("bias", (64,)), ("kernel", (64, 1))]
    assert leaves == want
    # inside a layer: batch_norm_f, batch_norm_s, batch_norm_out, then f, s (the reference's creation order)
    lay = m.conv_layers[0]
    subs = [s for s in lay.sublayers() if s.weights]
    want_subs = ([lay.batch_norm_f, lay.batch_norm_s, lay.batch_norm_out] if batch_norm else []) + [lay.f, lay.s]
    assert len(subs) == len(want_subs) and all(a is b for a, b in zip(subs, want_subs))
    assert m.fused_gate_layers == [True, True] and m.fused is None and m.auto_graph is True
    assert len(m.get_weights()) == len(want)
    # feature input and bare distances: widths follow
    m2 = CGCNN.make_crystal_model(
        inputs=[{"shape": (None, 7), "name": "node_attributes", "dtype": "float32", "ragged": True},
                {"shape": (None, 1), "name": "edge_distance", "dtype": "float32", "ragged": True},
                {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True}],
        make_distances=False, expand_distance=False, depth=1, conv_layer_args={"batch_normalization": False})
    assert [tuple(t.shape) for _, t in m2.weights][:3] == [(7, 64), (64,), (129, 64)]
    assert m2.fused_gate_layers == [True]


def test_fused_gate_supported_decisions():
    ok = dict(activation_s="softplus", activation_out="softplus", pooling_method="sum")
    assert FUSED_GATE_SIZES == {"units": 64, "max_edge_width": 64}
    assert fused_gate_supported(64, 64, 40, **ok)
    assert fused_gate_supported(64, 64, 1, **ok) and fused_gate_supported(64, 64, 64, **ok)
    assert not fused_gate_supported(64, 64, 65, **ok) and not fused_gate_supported(64, 64, 0, **ok)
    assert not fused_gate_supported(63, 63, 40, **ok) and not fused_gate_supported(128, 128, 40, **ok)
    assert not fused_gate_supported(64, 128, 40, **ok) and not fused_gate_supported(128, 64, 40, **ok)
    assert not fused_gate_supported(64, 64, 40, "softplus", "softplus", "mean")
    assert not fused_gate_supported(64, 64, 40, "softplus", "softplus", "sum", pooling_index=1)
    assert not fused_gate_supported(64, 64, 40, "gelu", "softplus", "sum")
    assert not fused_gate_supported(64, 64, 40, "softplus", "no_such_activation", "sum")
    assert fused_gate_supported(64, 64, 40, "swish", "linear", "sum")
    assert not fused_gate_supported(64, 64, 40, dtype="float64", **ok)
    # the layer decides in build()
    for units, width, edge, pooling, want in ((64, 64, 40, "sum", True), (63, 63, 40, "sum", False),
                                              (128, 128, 40, "sum", False), (64, 64, 65, "sum", False),
                                              (64, 64, 41, "mean", False)):
        lay = CGCNNLayer(units=units, pooling_method=pooling)
        lay.ensure_built([(None, None, width), (None, None, edge), (None, None, 2)])
        assert lay.fused_gate is want, (units, width, edge, pooling)
        assert tuple(lay.s.kernel.shape) == (2 * width + edge, units)


# ------------------------------------------------------------------------------------------------ the restatement, pinned
def _softplus(x):
    return np.log1p(np.exp(-np.abs(x))) + np.maximum(x, 0.0)


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


@pytest.mark.parametrize("batch_norm", [False, True])
def test_restatement_equals_a_per_edge_loop(batch_norm):
    """2 nodes, 3 edges, one of them from node 1 to its own image."""
    rng = np.random.default_rng(3)
    f_dim, bins = 4, 5
    frac = rng.uniform(0, 1, size=(2, 3))
    lattice = np.eye(3) * 3.0 + rng.uniform(-0.4, 0.4, size=(3, 3))        # the matrix A of the einsum
    ei = np.array([[0, 1], [1, 0], [1, 1]])
    trans = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, -1.0], [0.0, 1.0, 0.0]])
    h = rng.normal(size=(2, f_dim))
    gauss = {"bins": bins, "distance": 4.0, "sigma": 0.6, "offset": 0.1}
    w = {k: (rng.normal(size=(2 * f_dim + bins, f_dim)) * 0.4, rng.normal(size=f_dim) * 0.2) for k in ("f", "s")}
    for k in ("bn_f", "bn_s", "bn_out"):
        w[k] = (rng.uniform(0.5, 1.5, f_dim), rng.normal(size=f_dim) * 0.3, rng.normal(size=f_dim) * 0.3,
                rng.uniform(0.5, 2.0, f_dim)) if batch_norm else None
    # the loop
    dist = np.zeros((3, 1))
    for e, (i, j) in enumerate(ei):
        d = frac[i] - (frac[j] + trans[e])
        r = np.array([sum(d[jj] * lattice[k][jj] for jj in range(3)) for k in range(3)])    # 'ij,ikj->ik'
        dist[e, 0] = np.sqrt(np.sum(r * r))
    assert dist[2, 0] == pytest.approx(np.linalg.norm(lattice[:, 1]), rel=1e-14)          # the self image: column 1 of A

    def bn(x, v):
        if v is None:
            return x
        inv = v[0] / np.sqrt(v[3] + 1e-3)
        return x * inv + (v[1] - v[2] * inv)

    u, msgs = np.zeros((2, f_dim)), []
    for e, (i, j) in enumerate(ei):
        g = np.array([np.exp(-(dist[e, 0] - gauss["offset"] - k / bins * gauss["distance"]) ** 2 / (2 * 0.6 ** 2))
                      for k in range(bins)])
        x = np.concatenate([h[i], h[j], g])
        m = _softplus(bn(x @ w["s"][0] + w["s"][1], w["bn_s"])) * _sigmoid(bn(x @ w["f"][0] + w["f"][1], w["bn_f"]))
        msgs.append(m)
        u[i] += m
    want = _softplus(h + bn(u, w["bn_out"]))
    # the restatement
    tt = lambda a: None if a is None else tuple(torch.tensor(v) for v in a)
    d_ref = ref.edge_norm(ref.frac_to_real(ref.displacement_unit_cell(torch.tensor(frac), torch.tensor(ei),
                                                                      torch.tensor(trans)),
                                           torch.tensor(lattice)[None], [0, 3]))
    np.testing.assert_allclose(d_ref.numpy(), dist, rtol=1e-13)
    m_ref, h_ref = ref.cgcnn_layer(torch.tensor(h), ref.gauss_basis(d_ref, gauss, torch.float64), torch.tensor(ei),
                                   {k: tt(v) for k, v in w.items()})
    np.testing.assert_allclose(m_ref.numpy(), np.stack(msgs), rtol=1e-12)
    np.testing.assert_allclose(h_ref.numpy(), want, rtol=1e-12)


def _golden_batch(c, transposed=True):
    lat = c["lattice"].astype(np.float64)
    return {"node_frac_coordinates": c["xyz"].astype(np.float64) @ np.linalg.inv(lat),
            "lattice_matrix": (lat.T if transposed else lat)[None].copy(), "edge_indices": c["indices"],
            "cell_translations": c["images"].astype(np.float64), "node_splits": np.array([0, len(c["xyz"])]),
            "edge_splits": np.array([0, len(c["indices"])])}


@pytest.mark.parametrize("name", ["tri5_c40", "thin2_c40", "cubic1_c40"])
def test_restated_distances_equal_the_golden_ones_with_the_lattice_transposed(cases, name):
    c = cases[name]
    cfg = {"representation": "unit"}
    d = ref.edge_distances(_golden_batch(c), cfg, torch.float64).numpy().reshape(-1)
    err = float(np.max(np.abs(d - c["dist"])))
    print("[cgcnn] %s: distances off by %.2e A with the lattice transposed" % (name, err))
    assert err <= 1e-10            # float64 rounding through a 3x3 product, three orders of margin
    wrong = ref.edge_distances(_golden_batch(c, transposed=False), cfg, torch.float64).numpy().reshape(-1)
    if name != "cubic1_c40":       # a cubic lattice is symmetric: both conventions agree on it
        assert float(np.max(np.abs(wrong - c["dist"]))) > 1e-3
    else:
        assert np.array_equal(c["lattice"], c["lattice"].T)


def test_super_cell_gives_the_same_mean_pooled_output(cases):
    c = cases["tri5_c40"]
    xyz, lat = c["xyz"].astype(np.float64), c["lattice"].astype(np.float64)
    numbers = np.array([1, 6, 7, 8, 6])
    m = CGCNN.make_crystal_model(depth=2)
    assert m.config["node_pooling_args"]["pooling_method"] == "mean"
    p = list(synth.cgcnn_params(m, seed=5).values())

    def run(x, cell, z):
        idx, img, _ = pr.neighbours(x, cell, 4.0)
        b = {"node_number": z, "node_frac_coordinates": x @ np.linalg.inv(cell), "lattice_matrix": cell.T[None].copy(),
             "edge_indices": idx, "cell_translations": img.astype(np.float64), "node_splits": np.array([0, len(x)]),
             "edge_splits": np.array([0, len(idx)])}
        return ref.cgcnn_forward(p, b, m.config, dtype=torch.float64).numpy(), len(idx)

    a, m1 = run(xyz, lat, numbers)
    b, m2 = run(np.concatenate([xyz, xyz + lat[0]]), np.stack([2.0 * lat[0], lat[1], lat[2]]),
                np.concatenate([numbers, numbers]))
    assert m2 == 2 * m1 and a.shape == b.shape == (1, 1)
    err = float(np.max(np.abs(a - b)) / np.max(np.abs(a)))
    print("[identity] CGCNN super-cell: %.2e" % err)
    assert err <= 1e-12


def test_synth_cgcnn_batch_is_fractional_with_the_transposed_lattice(cases):
    s = synth.periodic_structures(num_graphs=3, seed=2)
    b = synth.cgcnn_batch(s)
    ns = b["node_splits"]
    for g in range(3):
        back = b["node_frac_coordinates"][ns[g]:ns[g + 1]].astype(np.float64) @ b["graph_lattice"][g].astype(np.float64)
        assert np.max(np.abs(back - b["node_coordinates"][ns[g]:ns[g + 1]])) <= 1e-5
        assert np.array_equal(b["lattice_matrix"][g], b["graph_lattice"][g].T)
    c = cases["thin2_c40"]
    one = {"node_number": np.array([1, 6]), "node_coordinates": c["xyz"], "node_splits": np.array([0, 2]),
           "graph_lattice": c["lattice"][None]}
    e = synth.cgcnn_batch(one, edges={"range_indices": c["indices"], "range_image": c["images"],
                                      "edge_splits": np.array([0, len(c["indices"])])})
    assert e["cell_translations"].dtype == np.float32 and e["edge_indices"].shape == (42, 2)
    d = ref.edge_distances(e, {"representation": "unit"}, torch.float64).numpy().reshape(-1)
    assert np.max(np.abs(d - c["dist"])) <= 1e-5       # float32 fractional coordinates
