"""MEGNet without a GPU: the crystal builder's defaults against the reference's dictionary, its refusals, weight names /
shapes / order, the ``MEGnetBlock`` config round trip, the decisions of ``fused_edge_supported``, the argument checks of
``mp_megnet_edge_f32``, the restatement (tests/megnet_reference.py) pinned against the NumPy oracle, and a check that the
named graph cases of the GPU tests cut tiles of 32 edges as they say."""
import numpy as np
import pytest
import torch

import megnet_reference as ref
import periodic_reference as pr
from gcnn_keras_amd import _ffi, synth
from gcnn_keras_amd.layers.conv.megnet_conv import FUSED_EDGE_SIZES, MEGnetBlock, fused_edge_supported
from gcnn_keras_amd.literature import Megnet
from oracle import kgcnn_oracle as ko

# kgcnn/literature/Megnet.py:196-219
REFERENCE_CRYSTAL_DEFAULT = {
    'name': "Megnet",
    'inputs': [{'shape': (None,), 'name': "node_attributes", 'dtype': 'float32', 'ragged': True},
               {'shape': (None, 3), 'name': "node_coordinates", 'dtype': 'float32', 'ragged': True},
               {'shape': (None, 2), 'name': "edge_indices", 'dtype': 'int64', 'ragged': True},
               {'shape': [1], 'name': "charge", 'dtype': 'float32', 'ragged': False},
               {'shape': (None, 3), 'name': "edge_image", 'dtype': 'int64', 'ragged': True},
               {'shape': (3, 3), 'name': "graph_lattice", 'dtype': 'float32', 'ragged': False}],
    'input_embedding': {"node": {"input_dim": 95, "output_dim": 64},
                        "graph": {"input_dim": 100, "output_dim": 64}},
    "make_distance": True, "expand_distance": True,
    'gauss_args': {"bins": 20, "distance": 4, "offset": 0.0, "sigma": 0.4},
    'meg_block_args': {'node_embed': [64, 32, 32], 'edge_embed': [64, 32, 32],
                       'env_embed': [64, 32, 32], 'activation': 'kgcnn>softplus2'},
    'set2set_args': {'channels': 16, 'T': 3, "pooling_method": "sum", "init_qstar": "0"},
    'node_ff_args': {"units": [64, 32], "activation": "kgcnn>softplus2"},
    'edge_ff_args': {"units": [64, 32], "activation": "kgcnn>softplus2"},
    'state_ff_args': {"units": [64, 32], "activation": "kgcnn>softplus2"},
    'nblocks': 3, 'has_ff': True, 'dropout': None, 'use_set2set': True,
    'verbose': 10,
    'output_embedding': 'graph',
    'output_mlp': {"use_bias": [True, True, True], "units": [32, 16, 1],
                   "activation": ['kgcnn>softplus2', 'kgcnn>softplus2', 'linear']}
}


@pytest.fixture(scope="module")
def cases(golden_dir):
    return pr.golden_cases(golden_dir)


# ------------------------------------------------------------------------------------------------ builder
def test_crystal_defaults_equal_the_reference():
    assert Megnet.model_crystal_default == REFERENCE_CRYSTAL_DEFAULT
    assert [i["name"] for i in Megnet.model_crystal_default["inputs"]] == [
        "node_attributes", "node_coordinates", "edge_indices", "charge", "edge_image", "graph_lattice"]
    assert Megnet.model_crystal_default["inputs"][4]["dtype"] == "int64"


@pytest.mark.parametrize("make", [Megnet.make_model, Megnet.make_crystal_model], ids=["molecular", "crystal"])
def test_builder_refusals(make):
    with pytest.raises(ValueError, match="Unsupported output embedding"):
        make(output_embedding="node")
    with pytest.raises(NotImplementedError, match="dropout"):
        make(dropout=0.1)
    with pytest.raises(ValueError):
        make(no_such_key=1)


def test_crystal_builder_needs_six_inputs():
    with pytest.raises(ValueError, match="six inputs"):
        Megnet.make_crystal_model(inputs=Megnet.model_default["inputs"])


def _mlp_weights(widths):
    out = []
    for k, (a, b) in enumerate(zip(widths[:-1], widths[1:])):
        out += [("mlp_dense_%d/kernel" % k, (a, b)), ("mlp_dense_%d/bias" % k, (b,))]
    return out


def _block_weights(fn, fe, fu):
    out = []
    for chain, width in (("lay_phi_n", 32 + fn + fu), ("lay_phi_e", 2 * fn + fe + fu), ("lay_phi_u", 32 + 32 + fu)):
        for k, (a, b) in enumerate(((width, 64), (64, 32), (32, 32))):
            out += [("dense/kernel", (a, b)), ("dense/bias", (b,))]
    return out


@pytest.mark.parametrize("state_embedding", [False, True])
def test_weight_names_shapes_and_order(state_embedding):
    inputs = list(Megnet.model_crystal_default["inputs"])
    if state_embedding:
        inputs[3] = {"shape": [], "name": "charge", "dtype": "float32", "ragged": False}
    m = Megnet.make_crystal_model(inputs=inputs)
    got = [(n, tuple(t.shape)) for n, t in m.weights]
    fu0 = 64 if state_embedding else 1
    want = [("embeddings", (95, 64))] + ([("embeddings", (100, 64))] if state_embedding else [])
    want += _mlp_weights([64, 64, 32]) + _mlp_weights([20, 64, 32]) + _mlp_weights([fu0, 64, 32])
    for i in range(3):
        if i > 0:
            want += _mlp_weights([32, 64, 32]) * 3
        want += _block_weights(32, 32, 32)
    want += [("kernel", (32, 16)), ("bias", (16,))] * 2
    want += [("lstm/kernel", (32, 64)), ("lstm/recurrent_kernel", (16, 64)), ("lstm/bias", (64,))] * 2
    want += _mlp_weights([96, 32, 16, 1])       # 2 x 2 x 16 Set2Set columns + 32 state
    assert [s for _, s in got] == [s for _, s in want]
    assert [n.rsplit("/", 1)[-1] for n, _ in got] == [n.rsplit("/", 1)[-1] for n, _ in want]
    # inside a block: the node chain, the edge chain, the state chain (the reference's attribute order)
    blk = m.blocks[0]
    subs = [s for s in blk.sublayers() if s.weights]
    chains = [blk.lay_phi_n, blk.lay_phi_n_1, blk.lay_phi_n_2, blk.lay_phi_e, blk.lay_phi_e_1, blk.lay_phi_e_2,
              blk.lay_phi_u, blk.lay_phi_u_1, blk.lay_phi_u_2]
    assert len(subs) == 9 and all(a is b for a, b in zip(subs, chains))
    assert m.fused_edge_blocks == [True] * 3 and m.use_fused_edge is True and m.auto_graph is True
    # the molecular builder creates the same layers in the same order
    mol = Megnet.make_model(inputs=inputs[:4])
    assert [tuple(t.shape) for _, t in mol.weights] == [s for _, s in got]
    assert mol.fused_edge_blocks == [True] * 3
    # has_ff=False drops the later triples only: the first one is always there, so every block still sees 32 / 32 / 32
    bare = Megnet.make_crystal_model(has_ff=False, nblocks=2)
    assert bare.fused_edge_blocks == [True, True]
    # other widths in front of the block stay on the layers
    wide = Megnet.make_crystal_model(node_ff_args={"units": [64, 64], "activation": "kgcnn>softplus2"}, nblocks=1)
    assert wide.fused_edge_blocks == [False]


def test_model_switch_is_a_property_over_the_blocks():
    m = Megnet.make_crystal_model(nblocks=2)
    m._graphs["x"] = [1, None, None]
    m.use_fused_edge = True                       # no change: the graphs stay
    assert "x" in m._graphs
    m.use_fused_edge = False
    assert m._graphs == {} and [b.use_fused_edge for b in m.blocks] == [False, False]
    m.blocks[0].use_fused_edge = True
    assert m.use_fused_edge is False


def test_block_config_round_trip_and_weight_gradients():
    kwargs = {"node_embed": [8, 9, 10], "edge_embed": [64, 32, 32], "env_embed": [5, 6, 7], "pooling_method": "sum",
              "use_bias": False, "activation": "swish"}
    blk = MEGnetBlock(**kwargs)
    config = blk.get_config()
    for k, v in kwargs.items():
        assert config[k] == v
    again = MEGnetBlock.from_config(config)
    assert again.get_config() == config
    assert MEGnetBlock.weight_gradients is True
    assert blk.use_fused_edge is True and blk.fused_edge is None     # decided in build()
    blk.ensure_built([(None, None, 32), (None, None, 32), (None, None, 2), (None, 32)])
    assert blk.fused_edge is True and [n.rsplit("/", 1)[-1] for n, _ in blk.weights] == ["kernel"] * 9


def test_fused_edge_supported_decisions():
    assert FUSED_EDGE_SIZES == {"node_width": 32, "edge_width": 32, "state_width": 32, "edge_embed": [64, 32, 32]}
    ok = dict(edge_embed=[64, 32, 32], activation="kgcnn>softplus2", pooling_method="mean")
    assert fused_edge_supported(32, 32, 32, **ok)
    assert fused_edge_supported(32, 32, 32, [64, 32, 32], "swish", "sum")
    assert fused_edge_supported(32, 32, 32, (64, 32, 32), None, "segment_mean")
    assert not fused_edge_supported(64, 32, 32, **ok)                                   # Fn = 64
    assert not fused_edge_supported(32, 20, 32, **ok) and not fused_edge_supported(32, 32, 1, **ok)
    assert not fused_edge_supported(32, 32, 32, [64, 32, 16], "kgcnn>softplus2", "mean")
    assert not fused_edge_supported(32, 32, 32, [64, 32, 32], "kgcnn>softplus2", "max")
    assert not fused_edge_supported(32, 32, 32, [64, 32, 32], "gelu", "mean")
    assert not fused_edge_supported(32, 32, 32, dtype="float64", **ok)
    for act in _ffi.ACTIVATION_CODES:
        assert fused_edge_supported(32, 32, 32, [64, 32, 32], act, "mean")
    # the block decides in build()
    for widths, embed, pooling, want in (((32, 32, 32), [64, 32, 32], "mean", True), ((32, 32, 32), [64, 32, 32], "sum", True),
                                         ((64, 32, 32), [64, 32, 32], "mean", False),
                                         ((32, 32, 32), [64, 32, 16], "mean", False),
                                         ((32, 32, 32), [64, 32, 32], "max", False)):
        blk = MEGnetBlock(edge_embed=embed, pooling_method=pooling)
        blk.ensure_built([(None, None, widths[0]), (None, None, widths[1]), (None, None, 2), (None, widths[2])])
        assert blk.fused_edge is want, (widths, embed, pooling)


# ------------------------------------------------------------------------------------------------ the C entry point
def _edge_args(**over):
    a = dict(Pa=None, Pb=None, N=4, Pu=None, splits=None, G=1, edges=None, Fn=32, Fe=32, Fu=32, cols=None, E=0, ptr0=None,
             perm0=None, Wc=None, W1=None, b1=None, W2=None, b2=None, u0=64, u1=32, u2=32, act=8, alpha=0.05, pool=_ffi.MP_MEAN,
             ws=None, ws_bytes=0, e_out=None, pool_out=None, stream=None)
    a.update(over)
    return list(a.values())


def test_edge_entry_point_argument_checks():
    lib = _ffi.lib()
    assert lib.mp_megnet_edge_f32(*_edge_args(Fn=16)) == _ffi.MP_EINVAL
    message = lib.mp_last_error()
    assert b"mp_megnet_edge_f32" in message and b"16" in message
    for bad in (dict(Fe=20), dict(Fu=1), dict(u2=16), dict(u0=128), dict(act=99), dict(act=-1), dict(pool=_ffi.MP_MAX),
                dict(N=-1), dict(E=2 ** 31), dict(N=2 ** 31)):
        assert lib.mp_megnet_edge_f32(*_edge_args(**bad)) == _ffi.MP_EINVAL, bad
        assert b"mp_megnet_edge_f32" in lib.mp_last_error()
    assert lib.mp_megnet_edge_f32(*_edge_args()) == _ffi.MP_EINVAL              # N > 0 with null pointers
    # zero-sized problems are accepted without touching the device
    assert lib.mp_megnet_edge_f32(*_edge_args(N=0)) == _ffi.MP_OK
    assert lib.mp_megnet_edge_f32(*_edge_args(N=0, G=0)) == _ffi.MP_OK
    import ctypes
    nbytes = ctypes.c_size_t(7)
    assert lib.mp_megnet_edge_ws_bytes(0, ctypes.byref(nbytes)) == _ffi.MP_OK and nbytes.value == 0
    assert lib.mp_megnet_edge_ws_bytes(33, ctypes.byref(nbytes)) == _ffi.MP_OK and nbytes.value == 2 * 2 * 32 * 4
    assert lib.mp_megnet_edge_ws_bytes(-1, ctypes.byref(nbytes)) == _ffi.MP_EINVAL


# ------------------------------------------------------------------------------------------------ the restatement, pinned
def _block_params(rng, fn, fe, fu, embeds):
    p, widths = {}, {"phi_e": 2 * fn + fe + fu, "phi_n": embeds["phi_e"][-1] + fn + fu,
                     "phi_u": embeds["phi_e"][-1] + embeds["phi_n"][-1] + fu}
    for name in ("phi_n", "phi_e", "phi_u"):
        a = widths[name]
        for suffix, b in zip(("", "_1", "_2"), embeds[name]):
            p["%s%s/kernel" % (name, suffix)] = rng.normal(size=(a, b)) * 0.3
            p["%s%s/bias" % (name, suffix)] = rng.normal(size=b) * 0.1
            a = b
    return p


@pytest.mark.parametrize("pooling", ["mean", "sum"])
def test_restated_block_equals_the_numpy_oracle(pooling):
    rng = np.random.default_rng(5)
    idx, ns, es = ref.multi_case(seed=2)
    n, e, g = int(ns[-1]), int(es[-1]), len(ns) - 1
    v, ed, u = rng.normal(size=(n, 6)), rng.normal(size=(e, 5)), rng.normal(size=(g, 4))
    p = _block_params(rng, 6, 5, 4, {"phi_n": [7, 8, 9], "phi_e": [10, 11, 12], "phi_u": [13, 14, 15]})
    rv, re_, ru = ko.megnet_block(ko.R(v, ns), ko.R(ed, es), ko.R(idx, es), u, p, pooling_method=pooling)
    w = {name: [(torch.tensor(p["%s%s/kernel" % (name, s)]), torch.tensor(p["%s%s/bias" % (name, s)]))
                for s in ("", "_1", "_2")] for name in ("phi_n", "phi_e", "phi_u")}
    flat = torch.from_numpy(ref.flat_edges({"edge_indices": idx, "node_splits": ns, "edge_splits": es}))
    gv, ge, gu = ref.megnet_block(torch.tensor(v), torch.tensor(ed), flat, torch.tensor(u), ref.graph_ids(ns),
                                  ref.graph_ids(es), w, pooling_method=pooling)
    np.testing.assert_allclose(ge.numpy(), re_.values, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(gv.numpy(), rv.values, rtol=1e-12, atol=1e-14)
    # the oracle's per-graph pools follow the reference's segment ops, which drop trailing empty graphs; `multi` ends in a
    # graph with nodes and edges, so every state row is there
    np.testing.assert_allclose(gu.numpy(), ru, rtol=1e-12, atol=1e-14)


def test_restated_molecular_forward_equals_the_numpy_oracle():
    b = synth.qm9_like_batch(num_graphs=4, seed=41)
    b["state"] = np.array([3, 0, 99, 5], np.float32)
    m = Megnet.make_model()
    p = [w.astype(np.float64) for w in synth.cgcnn_params(m, seed=3).values()]
    want = ko.megnet_forward(p, ko.R(b["node_number"], b["node_splits"]),
                             ko.R(b["node_coordinates"].astype(np.float64), b["node_splits"]),
                             ko.R(b["edge_indices"], b["edge_splits"]), b["state"])
    got = ref.megnet_forward(p, b, m.config, dtype=torch.float64, crystal=False).numpy()
    assert got.shape == want.shape == (4, 1)
    np.testing.assert_allclose(got, want, rtol=1e-10)


def test_restated_periodic_distances_equal_the_golden_ones(cases):
    for name in ("tri5_c40", "thin2_c40", "cubic1_c40"):
        c = cases[name]
        b = {"node_coordinates": c["xyz"].astype(np.float64), "graph_lattice": c["lattice"].astype(np.float64)[None],
             "edge_indices": c["indices"], "edge_image": c["images"], "node_splits": np.array([0, len(c["xyz"])]),
             "edge_splits": np.array([0, len(c["indices"])])}
        d = ref.periodic_distances(b, torch.float64).numpy().reshape(-1)
        assert np.max(np.abs(d - c["dist"])) <= 1e-10, name       # the lattice goes in untransposed (rows)


# ------------------------------------------------------------------------------------------------ the named cases cut tiles
def test_named_cases_cut_tiles_as_stated(cases):
    def segments(name):
        recv = cases[name]["indices"][:, 0]
        assert np.all(np.diff(recv) >= 0), name            # the golden lists are receiver-sorted
        deg = np.bincount(recv, minlength=len(cases[name]["xyz"]))
        starts = np.concatenate([[0], np.cumsum(deg)])
        return deg, [(int(a), int(b)) for a, b in zip(starts[:-1], starts[1:]) if b > a]

    deg, seg = segments("thin2_c40")
    assert deg.sum() == 42 and 32 < 42 < 64 and len(seg) == 2                                # crosses one tile edge
    assert len(cases["cubic1_c40"]["xyz"]) == 1
    assert np.all(cases["cubic1_c40"]["indices"] == 0) and np.all(np.any(cases["cubic1_c40"]["images"] != 0, axis=1))
    deg, _ = segments("big6_c40")
    assert np.sum(deg == 0) >= 2                                                             # isolated atoms
    _, seg = segments("tri5_c40")
    assert all(a // 32 != (b - 1) // 32 for a, b in seg)                                     # every receiver is cut
    _, seg = segments("tri5_c55")
    assert any((-(-a // 32) + 1) * 32 <= b for a, b in seg)                                  # one owns a whole tile
    for e in (0, 1, 31, 32, 33, 64, 65):
        idx, ns, es = ref.hand_case(e)
        assert idx.shape == (e, 2) and int(ns[-1]) == 4 and int(es[-1]) == e
        assert 2 not in idx[:, 0] and np.all(np.diff(idx[:, 0]) >= 0)
    idx, ns, es = ref.multi_case()
    assert list(es) == [0, 5, 5, 32, 33, 33, 73, 73, 76] and list(np.diff(ns)) == [3, 2, 4, 1, 0, 5, 2, 2]
    graph = np.repeat(np.arange(8), np.diff(es))
    assert set(graph[:32]) == {0, 2} and graph[31] == 2 and graph[32] == 3                   # tile 0, graph 2 ends at 32
    assert graph[63] == 5 and graph[64] == 5                                                 # graph 5 crosses 64
    for g in range(8):
        part = idx[es[g]:es[g + 1]]
        assert np.all(np.diff(part[:, 0]) >= 0) and (len(part) == 0 or part.max() < np.diff(ns)[g])
    shuffled, _, es2 = ref.multi_case(shuffled=True)
    assert np.array_equal(es, es2) and not np.array_equal(shuffled, idx)
    assert any(np.any(np.diff(shuffled[es[g]:es[g + 1], 0]) < 0) for g in range(8))          # the perm0 path runs
    idx, ns, es = ref.many_graphs_case(2100)
    assert len(ns) - 1 == 2100 > 2048 and int(ns[-1]) == 2100 and len(idx) == int(es[-1]) and es[-1] > es[-2]
    assert set(np.diff(es)) == {0, 1, 2}
    _, ns7, es7 = ref.multi_case(graphs=7)
    assert list(es7) == [0, 5, 5, 32, 33, 33, 73, 73] and es7[-1] == es7[-2] and ns7[-1] > ns7[-2]
