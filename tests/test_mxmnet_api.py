"""MXMNet without a GPU: the builder's dictionary against the reference's, configs, weight lists and the layers' quirks,
the route decisions, the declared entry points, both angle lists from their definitions, and the identities the GPU
tests rest on - the restatement (tests/mxmnet_reference.py) in float64 against central finite differences and under
rotation and translation, and its float32 twin within ``parity.BAR_CAP`` of float64 on the GPU tests' inputs."""
import ctypes

import numpy as np
import pytest
import torch

import mxmnet_reference as ref
from gcnn_keras_amd import _ffi, synth
from gcnn_keras_amd.layers.conv.mxmnet_conv import (MXMGlobalMP, MXMLocalMP, fused_step_supported,
                                                    fused_triplet_supported)
from gcnn_keras_amd.literature import MXMNet
from parity import BAR_CAP, rowwise_rel

F64 = torch.float64

# kgcnn/literature/MXMNet.py:24-53, as data
REFERENCE_DEFAULT = {
    "name": "MXMNet",
    "inputs": [{"shape": (None,), "name": "node_number", "dtype": "float32", "ragged": True},
               {"shape": (None, 3), "name": "node_coordinates", "dtype": "float32", "ragged": True},
               {"shape": (None,), "name": "edge_attributes", "dtype": "float32", "ragged": True},
               {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True},
               {"shape": [None, 2], "name": "angle_indices_1", "dtype": "int64", "ragged": True},
               {"shape": [None, 2], "name": "angle_indices_2", "dtype": "int64", "ragged": True},
               {"shape": (None, 2), "name": "range_indices", "dtype": "int64", "ragged": True}],
    "input_embedding": {"node": {"input_dim": 95, "output_dim": 32,
                                 "embeddings_initializer": {
                                     "class_name": "RandomUniform",
                                     "config": {"minval": -1.7320508075688772, "maxval": 1.7320508075688772}}},
                        "edge": {"input_dim": 32, "output_dim": 32}},
    "bessel_basis_local": {"num_radial": 16, "cutoff": 5.0, "envelope_exponent": 5},
    "bessel_basis_global": {"num_radial": 16, "cutoff": 5.0, "envelope_exponent": 5},
    "spherical_basis_local": {"num_spherical": 7, "num_radial": 6, "cutoff": 5.0, "envelope_exponent": 5},
    "mlp_rbf_kwargs": {"units": 32, "activation": "swish"},
    "mlp_sbf_kwargs": {"units": 32, "activation": "swish"},
    "global_mp_kwargs": {"units": 32},
    "local_mp_kwargs": {"units": 32, "output_units": 1, "output_kernel_initializer": "zeros"},
    "use_edge_attributes": False,
    "depth": 3,
    "verbose": 10,
    "node_pooling_args": {"pooling_method": "sum"},
    "output_embedding": "graph", "output_to_tensor": True,
    "use_output_mlp": True,
    "output_mlp": {"use_bias": [True], "units": [1], "activation": ["linear"]},
}

BASE_KEYS = {"name", "trainable", "dtype", "node_indexing", "ragged_validate", "is_sorted", "has_unconnected"}


# ------------------------------------------------------------------------------------------------------ the builder
def test_default_dictionary_is_the_references():
    assert MXMNet.model_default == REFERENCE_DEFAULT
    assert [type(i["shape"]) for i in MXMNet.model_default["inputs"]] == [tuple, tuple, tuple, tuple, list, list, tuple]
    assert MXMNet.__model_version__ == "2022.11.25"
    import gcnn_keras_amd.literature.MXMNet as module
    assert module is MXMNet
    m = MXMNet.make_model()
    assert m.name == "MXMNet" and m.auto_graph is True and m.__kgcnn_model_version__ == "2022.11.25"
    assert m.config["depth"] == 3 and m.config["global_mp_kwargs"] == {"units": 32}


def test_refusals():
    with pytest.raises(ValueError, match="Unsupported output embedding for mode `MXMNet`"):
        MXMNet.make_model(output_embedding="edge")
    with pytest.raises(ValueError, match="Unsupported output embedding"):
        MXMNet.make_model(output_embedding=None)
    with pytest.raises(ValueError):
        MXMNet.make_model(unknown_key=1)
    m = MXMNet.make_model()
    with pytest.raises(ValueError, match="expects"):
        m.set_weights([np.zeros((1, 1), np.float32)])
    with pytest.raises(ValueError, match="shared h_mlp"):
        MXMLocalMP(units=32).ensure_built([(None, None, 16), (None, None, 8), (None, None, 8), (None, None, 8),
                                           (None, None, 2), (None, None, 2), (None, None, 2)])


def test_layer_configs_round_trip():
    g = MXMGlobalMP(units=48, name="glob")
    assert set(g.get_config()) == BASE_KEYS | {"units"} and g.get_config()["units"] == 48
    again = MXMGlobalMP.from_config(g.get_config())
    assert again.get_config() == g.get_config() and again.dim == 48
    loc = MXMLocalMP(units=64, output_units=3, activation="swish", output_kernel_initializer="glorot_uniform",
                     pooling_method="mean", name="loc")
    conf = loc.get_config()
    assert set(conf) == BASE_KEYS | {"units", "output_units", "activation", "output_kernel_initializer",
                                     "pooling_method"}
    assert (conf["units"], conf["output_units"], conf["activation"], conf["output_kernel_initializer"],
            conf["pooling_method"]) == (64, 3, "swish", "glorot_uniform", "mean")
    again = MXMLocalMP.from_config(conf)
    assert again.get_config() == conf and again.y_W.kernel_initializer == "glorot_uniform"
    assert MXMLocalMP().get_config()["output_kernel_initializer"] == "zeros"
    assert (MXMGlobalMP().dim, MXMLocalMP().dim, MXMLocalMP().output_dim) == (64, 64, 1)


def _dense(fin, units, bias=True):
    return [(fin, units)] + ([(units,)] if bias else [])


def _residual(dim):
    return _dense(dim, dim) + _dense(dim, dim)


def _global_shapes(fin, dim, ka):
    return (_dense(fin, dim) + _residual(dim) * 3 + _dense(dim, dim)            # h_mlp, res1..3, mlp
            + _dense(2 * dim + ka, dim) + _dense(ka, dim, bias=False))          # x_edge_mlp, linear


def _local_shapes(dim, kr, ks, out):
    cat = 2 * dim + kr
    return (_dense(cat, dim) + _dense(cat, dim) + _dense(dim, dim) + _dense(dim, dim)     # mlp_kj, ji_1, ji_2, jj
            + (_dense(ks, dim) + _dense(dim, dim)) * 2                                    # mlp_sbf1, mlp_sbf2
            + _dense(kr, dim, bias=False) * 2 + _residual(dim) * 3                        # lin_rbf1/2, res1..3
            + _dense(kr, dim, bias=False)                                                 # lin_rbf_out
            + _dense(dim, dim)                                                            # h_mlp, after lin_rbf_out
            + _dense(dim, dim) * 3 + _dense(dim, out))                                    # y_mlp, y_W


def _model_shapes(width, depth, output_mlp):
    want = [(96, width), (16,), (16,)]                                # embedding, both Bessel frequency rows
    want += _dense(16, width) + _dense(42, width) * 2 + _dense(16, width)
    for _ in range(depth):
        want += _global_shapes(width, width, width) + _local_shapes(width, width, width, 1)
    return want + (_dense(1, 1) if output_mlp else [])


def test_weight_shapes_of_the_default_and_the_md17_configuration():
    m = MXMNet.make_model()
    assert [tuple(t.shape) for _, t in m.weights] == _model_shapes(32, 3, True)
    m = MXMNet.make_model(**synth.MXMNET_MD17)
    assert [tuple(t.shape) for _, t in m.weights] == _model_shapes(128, 6, False)
    assert len({id(t) for _, t in m.weights}) == len(m.weights)           # the shared h_mlp is listed once
    names = [n for n, _ in m.weights]
    assert len(set(names)) == len(names)                                  # a name-keyed load is unambiguous
    assert [type(x).__name__ for x in m.layers].count("MXMGlobalMP") == 6
    # edge attributes: the (embedded) input widens the local Bessel rows ahead of mlp_rbf
    m = MXMNet.make_model(use_edge_attributes=True)
    shapes = [tuple(t.shape) for _, t in m.weights]
    assert shapes[:2] == [(96, 32), (32, 32)] and (16 + 32, 32) in shapes
    m = MXMNet.make_model(**dict(synth.MXMNET_MD17, use_edge_attributes=True, depth=1))
    assert (16 + 1, 128) in [tuple(t.shape) for _, t in m.weights]
    # the node branch returns the embedded input through the output MLP: no message passing layer is part of it
    m = MXMNet.make_model(output_embedding="node")
    assert [tuple(t.shape) for _, t in m.weights] == [(96, 32), (32, 1), (1,)]
    assert [type(x).__name__ for x in m.layers] == ["EmbeddingDimeBlock", "MLP", "ChangeTensorType"]


def test_quirks_are_the_references():
    g = MXMGlobalMP(units=32)
    assert g.pool.pooling_method == "mean" and g.pool.pooling_index == 0          # PoolingLocalMessages() default
    loc = MXMLocalMP(units=32)
    assert {loc.pool_mkj.pooling_method, loc.pool_mjj.pooling_method, loc.pool_h.pooling_method} == {"sum"}
    assert MXMLocalMP(units=32, pooling_method="mean").pool_h.pooling_method == "mean"
    # h_mlp was assigned twice: one GraphMLP, listed where the second assignment stands (behind lin_rbf_out)
    subs = [s for s in loc.sublayers() if type(s).__name__ == "MLP"]
    assert sum(s is loc.h_mlp for s in subs) == 1
    order = [k for k, v in loc.__dict__.items() if any(v is s for s in loc.sublayers())]
    assert order.index("h_mlp") == order.index("lin_rbf_out") + 1 and order.index("y_mlp") == order.index("h_mlp") + 1
    loc.ensure_built([(None, None, 32), (None, None, 8), (None, None, 8), (None, None, 8), (None, None, 2),
                      (None, None, 2), (None, None, 2)])
    assert [tuple(t.shape) for _, t in loc.weights] == _local_shapes(32, 8, 8, 1)
    shared = [n for n, _ in loc.weights if n.startswith(loc.h_mlp.name + "/")]
    assert len(shared) == 2                                                       # one kernel, one bias
    # frozen weights, as DimeNet++: the layers carry no weight gradients and say so when asked for one
    assert MXMGlobalMP.weight_gradients is False and MXMLocalMP.weight_gradients is False
    assert not any(t.requires_grad for _, t in loc.weights)
    assert float(loc.y_W.kernel.abs().max()) == 0.0                               # output_kernel_initializer="zeros"


def test_train_on_batch_raises_and_leaves_the_weights_frozen():
    m = MXMNet.make_model(depth=1)
    m.compile(optimizer="sgd", loss="mean_squared_error")
    before = [t.clone() for t in m.trainable_weights]
    # the guard speaks before any kernel is reached: the inputs are not even looked at
    with pytest.raises(NotImplementedError, match="weight gradients are not implemented"):
        m.train_on_batch([torch.zeros(4)] * 7, np.zeros((1, 1), np.float32))
    assert not any(t.requires_grad for t in m.trainable_weights)
    assert all(torch.equal(a, c) for a, c in zip(before, m.trainable_weights))


def test_switch_is_part_of_the_model():
    m = MXMNet.make_model(depth=2)
    assert len(m.global_blocks) == 2 and len(m.local_blocks) == 2
    assert all(g.fused_step for g in m.global_blocks) and all(b.fused_step and b.fused_triplet for b in m.local_blocks)
    # the defaults: the global message and the triplet pools fused, the local per-edge messages not
    assert all(g.use_fused_step for g in m.global_blocks) and not m.use_fused_step
    assert all(b.use_fused_triplet and not b.use_fused_step for b in m.local_blocks)
    m.use_fused_step = False
    assert not m.use_fused_step
    assert not any(g.use_fused_step for g in m.global_blocks)
    assert not any(b.use_fused_step or b.use_fused_triplet for b in m.local_blocks)
    m.use_fused_step = True
    assert m.use_fused_step and all(b.use_fused_step and b.use_fused_triplet for b in m.local_blocks)
    m.local_blocks[1].use_fused_triplet = False
    assert not m.use_fused_step and not m.shipped_routes
    m.use_fused_step = None                                   # back to the mix the model was built with
    assert m.shipped_routes and not m.use_fused_step and all(g.use_fused_step for g in m.global_blocks)
    assert all(b.use_fused_triplet and not b.use_fused_step for b in m.local_blocks)


def test_route_decisions():
    for units in (32, 64, 128):
        for ka in (1, 5, 32, 128):
            assert fused_step_supported(units, ka, "swish", "mean")
    for name in ("relu", "tanh", "sigmoid", "kgcnn>swish", "linear", None, "softplus", "selu"):
        assert fused_step_supported(32, 16, name)
    for bad in (dict(units=48), dict(units=16), dict(units=256), dict(edge_width=0), dict(edge_width=129),
                dict(edge_width=None), dict(activation="elu"), dict(activation="softmax"), dict(pooling_method="max"),
                dict(dtype="float64"), dict(dtype=torch.float64)):
        kw = dict(dict(units=32, edge_width=16, activation="swish", pooling_method="sum"), **bad)
        assert not fused_step_supported(**kw), bad
    assert fused_triplet_supported("sum") and fused_triplet_supported("mean")
    assert not fused_triplet_supported("max") and not fused_triplet_supported("sum", "float64")
    # the layers decide in build()
    shapes = lambda f, ka: [(None, None, f), (None, None, ka), (None, None, 2)]
    g = MXMGlobalMP(units=64)
    assert g.fused_step is None and g.use_fused_step
    assert g.ensure_built(shapes(64, 16)).fused_step is True
    assert MXMGlobalMP(units=48).ensure_built(shapes(48, 16)).fused_step is False
    assert MXMGlobalMP(units=32).ensure_built(shapes(32, 129)).fused_step is False
    local = lambda dim, kr: [(None, None, dim), (None, None, kr), (None, None, 7), (None, None, 7), (None, None, 2),
                             (None, None, 2), (None, None, 2)]
    loc = MXMLocalMP(units=32).ensure_built(local(32, 16))
    assert loc.fused_step is True and loc.fused_triplet is True
    loc = MXMLocalMP(units=48, pooling_method="max").ensure_built(local(48, 16))
    assert loc.fused_step is False and loc.fused_triplet is False
    assert MXMLocalMP(units=32, activation="elu").ensure_built(local(32, 16)).fused_step is False


# ------------------------------------------------------------------------------------------------ the C entry points
NEW_SYMBOLS = ["mp_mxm_edge_f32", "mp_mxm_edge_grad_f32", "mp_mxm_edge_ws_bytes", "mp_mxm_triplet_f32",
               "mp_mxm_triplet_grad_f32"]


def test_entry_points_are_declared_behind_the_umbrella():
    assert [n for n in _ffi.declared_symbols() if n.startswith("mp_mxm")] == NEW_SYMBOLS
    assert len(_ffi._SIGNATURES) == 198 and not any(n in _ffi._SIGNATURES for n in NEW_SYMBOLS)
    assert "mpengine/mxmnet.h" in _ffi.FAMILY_HEADERS and sorted(_ffi._FAMILY_SIGNATURES) == NEW_SYMBOLS
    assert all(("int %s(" % n) in _ffi.HEADER_TEXT for n in NEW_SYMBOLS)
    P, i, i64, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    sig = _ffi._FAMILY_SIGNATURES
    assert sig["mp_mxm_edge_ws_bytes"] == [i64, i, P]
    assert sig["mp_mxm_edge_f32"] == [P, P, i64, i, P, i, P, P, P, P, i64, P, P, i, f, i, P, P, ctypes.c_size_t, P, P, P,
                                      P, P]
    assert sig["mp_mxm_edge_grad_f32"] == [P, i, i64, i, i, P, P, P, i64, P, i, f, i, P, P, P, P, P]
    assert sig["mp_mxm_triplet_f32"] == [P, i64, i, P, P, i64, P, P, i, P, P]
    assert sig["mp_mxm_triplet_grad_f32"] == [P, i64, i, P, P, i64, P, P, P, i, P, P, P, P]
    lib = _ffi.lib()
    assert lib.mp_mxm_edge_f32.argtypes == sig["mp_mxm_edge_f32"] and lib.mp_mxm_edge_f32.restype is ctypes.c_int


def _edge_args(n=4, w=32, ka=8, e=0, act=4, op=None, ws_bytes=0, out=True):
    one = ctypes.c_void_p(16)
    return [None, None, n, w, None, ka, None, None, None, None, e, None, None, act, 0.05,
            _ffi.MP_MEAN if op is None else op, None, None, ws_bytes, None, None, one if out else None,
            None if out else one, None]


def test_argument_checks():
    lib = _ffi.lib()
    fn = lib.mp_mxm_edge_f32
    for bad, word in ((dict(w=48), b"width"), (dict(w=0), b"width"), (dict(w=256), b"width"),
                      (dict(ka=0), b"attribute width"), (dict(ka=129), b"attribute width"),
                      (dict(act=-1), b"activation"), (dict(act=_ffi.MP_ACT_LAST + 1), b"activation"),
                      (dict(op=_ffi.MP_MAX), b"pooling"), (dict(n=-1), b"sizes"), (dict(e=2 ** 31 - 32), b"sizes")):
        assert fn(*_edge_args(**bad)) == _ffi.MP_EINVAL, bad
        message = lib.mp_last_error()
        assert b"mp_mxm_edge_f32" in message and word in message, (bad, message)
    assert fn(*_edge_args(n=0)) == _ffi.MP_OK                                  # no nodes: nothing to do, no device
    assert fn(*_edge_args(n=4, e=0, out=False)) == _ffi.MP_OK                  # edge epilogue without edges
    both = _edge_args()
    both[22] = both[21]
    assert fn(*both) == _ffi.MP_EINVAL and b"exactly one" in lib.mp_last_error()
    assert fn(*_edge_args(n=4, e=8)) == _ffi.MP_EINVAL and b"null pointer" in lib.mp_last_error()
    with pytest.raises(ValueError, match="mp_mxm_edge_f32"):
        _ffi.call("mp_mxm_edge_f32", *_edge_args(w=48))
    grad = lib.mp_mxm_edge_grad_f32
    assert grad(None, 1, 4, 48, 8, None, None, None, 8, None, 4, 0.05, _ffi.MP_SUM, None, None, None, None,
                None) == _ffi.MP_EINVAL
    assert grad(None, 1, 4, 32, 8, None, None, None, 0, None, 4, 0.05, _ffi.MP_SUM, None, None, None, None,
                None) == _ffi.MP_OK
    trip = lib.mp_mxm_triplet_f32
    assert trip(None, 0, 32, None, None, 0, None, None, _ffi.MP_SUM, None, None) == _ffi.MP_OK
    assert trip(None, 4, 32, None, None, 0, None, None, _ffi.MP_MAX, None, None) == _ffi.MP_EINVAL
    assert trip(None, 4, 0, None, None, 0, None, None, _ffi.MP_SUM, None, None) == _ffi.MP_EINVAL
    assert trip(None, 4, 32, None, None, 0, None, None, _ffi.MP_SUM, None, None) == _ffi.MP_EINVAL     # null ptr0
    for e, w, want in ((0, 32, 0), (1, 32, 256), (32, 64, 512), (33, 64, 1024), (65, 128, 3 * 2 * 128 * 4)):
        assert _ffi.workspace_bytes("mp_mxm_edge_ws_bytes", e, w) == want
    with pytest.raises(ValueError, match="mp_mxm_edge_ws_bytes"):
        _ffi.workspace_bytes("mp_mxm_edge_ws_bytes", 4, 48)


# ------------------------------------------------------------------------------------------------ angle lists
def test_angle_lists_from_their_definitions():
    edi = np.array([[0, 1], [0, 2], [1, 0], [1, 2], [2, 0], [2, 1]])
    jk, ik = ref.angle_lists(edi)
    # n = (i, j) with m = (j, k), k != i
    assert jk.tolist() == [[0, 3], [1, 5], [2, 1], [3, 4], [4, 0], [5, 2]]
    # n = (i, j) with itself and with every m = (i, k), k != j
    assert ik.tolist() == [[0, 0], [0, 1], [1, 0], [1, 1], [2, 2], [2, 3], [3, 2], [3, 3], [4, 4], [4, 5], [5, 4], [5, 5]]
    assert np.all(edi[jk[:, 0], 1] == edi[jk[:, 1], 0]) and np.all(edi[ik[:, 0], 0] == edi[ik[:, 1], 0])
    lone = ref.angle_lists(np.array([[0, 1]]))
    assert lone[0].shape == (0, 2) and lone[1].tolist() == [[0, 0]]
    empty = ref.angle_lists(np.zeros((0, 2), np.int64))
    assert empty[0].shape == (0, 2) and empty[1].shape == (0, 2)
    for which in ("default", "md17"):
        b = ref.model_batch(which, synth)
        es, s1, s2 = b["edge_splits"], b["angle_splits_1"], b["angle_splits_2"]
        for g in range(len(es) - 1):
            jk, ik = ref.angle_lists(b["edge_indices"][es[g]:es[g + 1]])
            np.testing.assert_array_equal(b["angle_indices_1"][s1[g]:s1[g + 1]], jk)
            np.testing.assert_array_equal(b["angle_indices_2"][s2[g]:s2[g + 1]], ik)
            np.testing.assert_array_equal(synth.angle_pairs(b["edge_indices"][es[g]:es[g + 1]], "jk"), jk)
        assert np.sum(b["angle_indices_2"][:, 0] == b["angle_indices_2"][:, 1]) == len(b["edge_indices"])


def test_model_batches_meet_both_cutoffs():
    for which, local in (("default", 2.0), ("md17", 3.0)):
        b = ref.model_batch(which, synth)
        ns = b["node_splits"]
        assert np.diff(ns).tolist() == ref.MODEL_SIZES
        x = b["node_coordinates"].astype(np.float64)
        dist = np.concatenate([synth.distance_matrix(x[ns[g]:ns[g + 1]])[np.triu_indices(ns[g + 1] - ns[g], 1)]
                               for g in range(len(ns) - 1)])
        assert dist.min() >= 0.8
        assert np.any(dist >= 5.0) and np.any((dist >= local) & (dist < 5.0)) and np.any(dist < local)
        assert len(b["angle_indices_1"]) > 0 and len(b["range_indices"]) > len(b["edge_indices"]) > 0


# ------------------------------------------------------------------------------------------------ the restatement
def _small_model():
    cfg = ref.model_config("default", synth, MXMNet)
    cfg.update(depth=2)
    m = MXMNet.make_model(**cfg)
    return m, list(synth.mxmnet_params(m, seed=7).values())


def test_restatement_forces_match_finite_differences():
    b = synth.mxmnet_batch(sizes=[4, 6], seed=4, min_distance=0.9, local_distance=2.5)
    m, p = _small_model()
    _, force = ref.energy_forces(p, b, m)
    assert float(force.abs().max()) > 1e-4
    x0 = torch.tensor(b["node_coordinates"], dtype=F64)
    h = 1e-6
    for atom, comp in ((0, 0), (2, 2), (5, 1), (9, 0)):
        xp, xm = x0.clone(), x0.clone()
        xp[atom, comp] += h
        xm[atom, comp] -= h
        ep = ref.mxmnet_forward(p, b, m, xyz=xp).sum()
        em = ref.mxmnet_forward(p, b, m, xyz=xm).sum()
        fd = -(ep - em).item() / (2 * h)
        assert abs(fd - force[atom, comp].item()) <= 1e-6 * max(float(force.abs().max()), abs(fd))


def test_restatement_is_invariant_under_rotation_and_translation():
    b = synth.mxmnet_batch(sizes=[4, 6], seed=4, min_distance=0.9, local_distance=2.5)
    m, p = _small_model()
    e0, f0 = ref.energy_forces(p, b, m)
    q, _ = np.linalg.qr(np.random.default_rng(14).normal(size=(3, 3)))
    b2 = dict(b)
    b2["node_coordinates"] = b["node_coordinates"].astype(np.float64) @ q.T + np.array([0.7, -1.3, 2.1])
    e1, f1 = ref.energy_forces(p, b2, m)
    assert float((e1 - e0).abs().max()) <= 1e-10 * max(1.0, float(e0.abs().max()))
    assert np.max(np.abs(f1.numpy() - f0.numpy() @ q.T)) <= 1e-9 * float(f0.abs().max())


def test_restatement_layers_agree_with_the_model_pieces():
    """The stand-alone edge message and triplet pool of the restatement are what its layers compute."""
    rng = np.random.default_rng(5)
    g = MXMGlobalMP(units=8).ensure_built([(None, None, 8), (None, None, 5), (None, None, 2)])
    ws = [rng.normal(size=tuple(t.shape)) * 0.3 for _, t in g.weights]
    x, a = torch.tensor(rng.normal(size=(6, 8))), torch.tensor(rng.normal(size=(9, 5)))
    ri = torch.from_numpy(rng.integers(0, 6, size=(9, 2)))
    table = ref.weights_of(g, ws)
    dense = g.x_edge_mlp.mlp_dense_layer_list[0]
    direct = ref.edge_message(x, a, ri, torch.tensor(table[id(dense.kernel)]), torch.tensor(table[id(dense.bias)]),
                              torch.tensor(table[id(g.linear.kernel)]), "swish", "mean", base=x)
    assert float((direct - ref.propagate(g, ws, x, a, ri)).abs().max()) <= 1e-12
    pairs = torch.from_numpy(rng.integers(0, 9, size=(20, 2)))
    s = torch.tensor(rng.normal(size=(20, 5)))
    want = torch.zeros(9, 5, dtype=F64)
    for t in range(20):
        want[pairs[t, 0]] += a[pairs[t, 1]] * s[t]
    assert float((ref.triplet_pool(a, s, pairs, "sum") - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("which", ["default", "md17"])
def test_float32_restatement_is_within_the_cap_of_float64(which):
    """The inputs and weight draws of the GPU tests: output rows and every molecule's forces, float32 against float64,
    inside ``BAR_CAP``."""
    b = ref.model_batch(which, synth)
    m = MXMNet.make_model(**ref.model_config(which, synth, MXMNet))
    p = list(synth.mxmnet_params(m, seed=ref.WEIGHT_SEED).values())
    e64, f64 = ref.energy_forces(p, b, m, F64)
    e32, f32 = ref.energy_forces(p, b, m, torch.float32)
    assert e64.shape == (len(ref.MODEL_SIZES), 1) and float(e64.abs().min()) > 1e-3
    err = rowwise_rel(e32.numpy(), e64.numpy())
    ns, worst = b["node_splits"], 0.0
    for g in range(len(ns) - 1):
        a, c = f32.numpy()[ns[g]:ns[g + 1]], f64.numpy()[ns[g]:ns[g + 1]]
        assert np.abs(c).max() > 1e-4
        worst = max(worst, float(np.abs(a - c).max() / np.abs(c).max()))
    print("[mxmnet] %s: float32 restatement %.2e (rows), %.2e (forces, worst molecule) from float64" % (which, err, worst))
    assert err <= BAR_CAP and worst <= BAR_CAP
