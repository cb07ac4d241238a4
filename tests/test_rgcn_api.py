"""RGCN and GNNFilm without a GPU: the builders' defaults, weights and refusals, ``RelationalDense`` with ``num_bases`` /
``num_blocks``, the route decisions, config round trips, and the pins of the torch restatement
(tests/rgcn_reference.py) that the GPU parity tests lean on - one block of each model against a per-edge NumPy loop, and
the identity the fused kernel computes (the edge sum in front of the per-relation product) against it in float64."""
import numpy as np
import pytest
import torch

import rgcn_reference as ref
from gcnn_keras_amd import synth
from gcnn_keras_amd.layers.conv.rgcn_conv import GNNFilmStep, RGCNStep, fused_relational_supported
from gcnn_keras_amd.layers.relational import DecomposedRelationalDense, RelationalDense
from gcnn_keras_amd.literature import GNNFilm, RGCN
from parity import rowwise_rel


# ------------------------------------------------------------------------------------------------------------ config
def test_model_defaults_are_the_reference_configuration():
    assert RGCN.__model_version__ == "2022.11.25" and GNNFilm.__model_version__ == "2022.11.25"
    assert RGCN.model_default == {
        "name": "RGCN",
        "inputs": [{"shape": (None,), "name": "node_attributes", "dtype": "float32", "ragged": True},
                   {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True},
                   {"shape": (None, 1), "name": "edge_weights", "dtype": "float32", "ragged": True},
                   {"shape": (None,), "name": "edge_relations", "dtype": "int64", "ragged": True}],
        "input_embedding": {"node": {"input_dim": 95, "output_dim": 64}},
        "dense_relation_kwargs": {"units": 64, "num_relations": 20},
        "dense_kwargs": {"units": 64},
        "activation_kwargs": {"activation": "swish"},
        "depth": 3, "verbose": 10,
        "output_embedding": "graph", "output_to_tensor": True,
        "output_mlp": {"use_bias": True, "units": 1, "activation": "softmax"},
    }
    assert GNNFilm.model_default == {
        "name": "GNNFilm",
        "inputs": [{"shape": (None,), "name": "node_attributes", "dtype": "float32", "ragged": True},
                   {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True},
                   {"shape": (None,), "name": "edge_relations", "dtype": "int64", "ragged": True}],
        "input_embedding": {"node": {"input_dim": 95, "output_dim": 64}},
        "dense_relation_kwargs": {"units": 64, "num_relations": 20},
        "dense_modulation_kwargs": {"units": 64, "num_relations": 20, "activation": "sigmoid"},
        "activation_kwargs": {"activation": "swish"},
        "depth": 3, "verbose": 10,
        "output_embedding": "graph", "output_to_tensor": True,
        "output_mlp": {"use_bias": True, "units": 1, "activation": "softmax"},
    }


def test_config_round_trips():
    step = RGCNStep(dense_kwargs={"units": 32, "activation": "relu"},
                    dense_relation_kwargs={"units": 32, "num_relations": 7, "num_bases": 2, "use_bias": False},
                    activation_kwargs={"activation": "tanh"})
    conf = step.get_config()
    assert conf["dense_kwargs"] == {"units": 32, "activation": "relu"}
    assert conf["dense_relation_kwargs"] == {"units": 32, "num_relations": 7, "num_bases": 2, "use_bias": False}
    assert conf["activation_kwargs"] == {"activation": "tanh"}
    assert RGCNStep.from_config(conf).get_config() == conf
    film = GNNFilmStep(dense_relation_kwargs={"units": 32, "num_relations": 4, "num_blocks": 2},
                       dense_modulation_kwargs={"units": 32, "num_relations": 4, "activation": "tanh"},
                       activation_kwargs={"activation": "relu"})
    conf = film.get_config()
    assert conf["dense_modulation_kwargs"] == {"units": 32, "num_relations": 4, "activation": "tanh"}
    assert GNNFilmStep.from_config(conf).get_config() == conf
    rd = DecomposedRelationalDense(8, num_relations=4, num_bases=2, num_blocks=2, activation="tanh")
    conf = rd.get_config()
    assert conf["num_bases"] == 2 and conf["num_blocks"] == 2 and conf["units"] == 8 and conf["num_relations"] == 4
    assert DecomposedRelationalDense.from_config(conf).get_config() == conf


# ----------------------------------------------------------------------------------------------------------- weights
def _leaves(weights):
    return [(n.rsplit("/", 1)[-1], tuple(t.shape)) for n, t in weights]


def test_relational_dense_weights_for_bases_and_blocks():
    shape = [(None, None, 12), (None, None)]
    # the plain class keeps its kernel and its refusal (tests/test_hdnnp_api.py); the subclass serves both options
    assert _leaves(RelationalDense(8, num_relations=5).ensure_built(shape).weights) == [("kernel", (5, 12, 8)),
                                                                                         ("bias", (8,))]
    for kw in ({"num_bases": 2}, {"num_blocks": 2}):
        with pytest.raises(NotImplementedError, match="DecomposedRelationalDense"):
            RelationalDense(8, num_relations=5, **kw)
    assert issubclass(DecomposedRelationalDense, RelationalDense)
    plain = DecomposedRelationalDense(8, num_relations=5).ensure_built(shape)
    assert _leaves(plain.weights) == [("kernel", (5, 12, 8)), ("bias", (8,))]
    bases = DecomposedRelationalDense(8, num_relations=5, num_bases=3).ensure_built(shape)
    assert _leaves(bases.weights) == [("kernel", (3, 12, 8)), ("lin_bases", (5, 3)), ("bias", (8,))]
    blocks = DecomposedRelationalDense(8, num_relations=5, num_blocks=4, use_bias=False).ensure_built(shape)
    assert _leaves(blocks.weights) == [("kernel", (5, 4, 3, 2))]
    both = DecomposedRelationalDense(8, num_relations=5, num_bases=3, num_blocks=2).ensure_built(shape)
    assert _leaves(both.weights) == [("kernel", (3, 2, 6, 4)), ("lin_bases", (5, 3)), ("bias", (8,))]
    assert both.weight_gradients is True
    with pytest.raises(AssertionError, match="num_blocks"):
        DecomposedRelationalDense(8, num_relations=5, num_blocks=5).ensure_built(shape)
    # every multi-kernel slice on its own fan: (12, 8) -> limit sqrt(6 / 20), never the stacked tensor's
    limit = np.sqrt(6.0 / 20.0)
    for lay in (plain, bases):
        k = lay.kernel.numpy()
        assert np.max(np.abs(k)) <= limit and np.max(np.abs(k)) > 0.8 * limit


def test_default_model_weights_names_shapes_order():
    model = RGCN.make_model()
    assert _leaves(model.weights) == ([("embeddings", (95, 64))]
                                      + [("kernel", (64, 64)), ("bias", (64,)), ("kernel", (20, 64, 64)), ("bias", (64,))] * 3
                                      + [("kernel", (64, 1)), ("bias", (1,))])
    names = [n for n, _ in model.weights]
    assert "dense" in names[1] and "relational_dense" in names[3]         # Dense first, then RelationalDense
    assert len({n.split("/", 1)[0] for n in names[1:13]}) == 3             # new layers in every block
    assert model.auto_graph is True and model.use_fused_relational is True
    assert model.fused_relational_blocks == [True] * 3
    assert model.__kgcnn_model_version__ == "2022.11.25"
    assert all(t is not None for _, t in model.weights)
    model.set_weights(list(synth.relational_params(model).values()))

    film = GNNFilm.make_model()
    assert _leaves(film.weights) == ([("embeddings", (95, 64))]
                                     + [("kernel", (20, 64, 64)), ("bias", (64,))] * 9
                                     + [("kernel", (64, 1)), ("bias", (1,))])
    assert film.auto_graph is True and film.use_fused_relational is True and film.fused_relational_blocks == [True] * 3
    assert film.__kgcnn_model_version__ == "2022.11.25"
    film.set_weights(list(synth.relational_params(film).values()))


def test_model_variants_build():
    rel = {"units": 64, "num_relations": 20, "num_bases": 3, "num_blocks": 2}
    m = RGCN.make_model(depth=2, dense_relation_kwargs=rel)
    block = _leaves(m.weights)[1:6]
    assert block == [("kernel", (64, 64)), ("bias", (64,)), ("kernel", (3, 2, 32, 32)), ("lin_bases", (20, 3)),
                     ("bias", (64,))]
    assert m.fused_relational_blocks == [True, True]
    m = GNNFilm.make_model(depth=1, dense_relation_kwargs=rel, output_embedding="node")
    assert _leaves(m.weights)[1:8] == [("kernel", (20, 64, 64)), ("bias", (64,))] * 2 + \
        [("kernel", (3, 2, 32, 32)), ("lin_bases", (20, 3)), ("bias", (64,))]
    spec = [dict(s) for s in RGCN.model_default["inputs"]]
    spec[0]["shape"] = (None, 32)
    m = RGCN.make_model(inputs=spec, depth=2, dense_kwargs={"units": 128},
                        dense_relation_kwargs={"units": 128, "num_relations": 4})
    assert _leaves(m.weights)[:2] == [("kernel", (32, 128)), ("bias", (128,))]
    assert _leaves(m.weights)[6] == ("kernel", (4, 128, 128)) and m.fused_relational_blocks == [True, True]


def test_synth_relational_batch():
    b = synth.relational_batch(7, seed=3, num_relations=5)
    again = synth.relational_batch(7, seed=3, num_relations=5)
    assert all(np.array_equal(b[k], again[k]) for k in b)
    m = int(b["edge_splits"][-1])
    assert b["edge_relations"].shape == (m,) and b["edge_relations"].dtype == np.int64
    assert b["edge_relations"].min() >= 0 and b["edge_relations"].max() < 5 and len(set(b["edge_relations"])) == 5
    assert b["edge_weights"].shape == (m, 1) and b["edge_weights"].dtype == np.float32
    es = b["edge_splits"]
    for g in range(7):
        rel, rev = b["edge_relations"][es[g]:es[g + 1]], b["edge_indices_reverse"][es[g]:es[g + 1], 0]
        assert np.array_equal(rel[rev], rel)                       # both directions of a bond share the relation


# ------------------------------------------------------------------------------------------ refusals, route decisions
def test_builders_refuse_other_embeddings():
    with pytest.raises(ValueError, match="Unsupported output embedding for mode `RGCN`"):
        RGCN.make_model(output_embedding="edge")
    with pytest.raises(ValueError, match="Unsupported output embedding for mode `GNNFilm`"):
        GNNFilm.make_model(output_embedding="edge")


def test_supported_decisions():
    for k in (32, 64, 128):
        for u in (32, 64, 128):
            for r in (1, 20, 64):
                assert fused_relational_supported(k, u, r, "linear", ("swish", None, "sigmoid"))
                assert fused_relational_supported(k, u, r, None, ("relu",), edge_weight_width=1)
    assert not fused_relational_supported(64, 64, 65)                                  # the relation mask has 64 bits
    assert not fused_relational_supported(64, 64, 0)
    assert not fused_relational_supported(48, 64, 20) and not fused_relational_supported(64, 48, 20)
    assert not fused_relational_supported(64, 64, 20, "relu")                          # the message has to be linear
    assert not fused_relational_supported(64, 64, 20, edge_weight_width=64)
    assert not fused_relational_supported(64, 64, 20, "linear", ("elu",))
    assert not fused_relational_supported(64, 64, 20, dtype="float64")
    # the decision is taken at build
    assert RGCN.make_model(depth=2).fused_relational_blocks == [True, True]
    rel = lambda **kw: dict({"units": 64, "num_relations": 20}, **kw)
    assert RGCN.make_model(depth=1, dense_relation_kwargs=rel(num_relations=65)).fused_relational_blocks == [False]
    assert RGCN.make_model(depth=1, dense_relation_kwargs=rel(activation="relu")).fused_relational_blocks == [False]
    assert RGCN.make_model(depth=1, dense_relation_kwargs=rel(use_bias=False)).fused_relational_blocks == [True]
    spec = [dict(s) for s in RGCN.model_default["inputs"]]
    spec[2]["shape"] = (None, 64)
    assert RGCN.make_model(depth=1, inputs=spec).fused_relational_blocks == [False]
    spec = [dict(s) for s in GNNFilm.model_default["inputs"]]
    spec[0]["shape"] = (None, 48)
    assert GNNFilm.make_model(depth=2, inputs=spec).fused_relational_blocks == [False, True]
    mod = {"units": 64, "num_relations": 20, "activation": "elu"}
    assert GNNFilm.make_model(depth=1, dense_modulation_kwargs=mod).fused_relational_blocks == [False]
    m = GNNFilm.make_model(depth=2)
    m.use_fused_relational = False
    assert m.use_fused_relational is False and all(not lay.use_fused_relational for lay in m.relational_layers)
    m.use_fused_relational = True
    assert m.use_fused_relational is True


def test_entry_point_refusals():
    """Argument errors and the empty problem need no device."""
    from gcnn_keras_amd import _ffi
    lib = _ffi.lib()
    args = lambda k, u, r, n=0: (0, None, n, k, None, 0, None, None, None, None, r, None, None, u, None, None, 0, None,
                                 None, None, None, 0, 0, 0.0, None, None)
    assert lib.mp_relational_conv_f32(*args(64, 64, 20)) == _ffi.MP_OK                 # N = 0: no launch
    for bad in (args(48, 64, 20), args(64, 256, 20), args(64, 64, 65), args(64, 64, 0)):
        assert lib.mp_relational_conv_f32(*bad) == _ffi.MP_EINVAL
        assert b"mp_relational_conv_f32" in lib.mp_last_error()
    assert lib.mp_relational_conv_f32(*args(64, 64, 20, n=4)) == _ffi.MP_EINVAL          # rows and no pointers


# -------------------------------------------------------------------------------------------- pins of the restatement
def _tiny(seed=3, k=5, u=4, r=3):
    rng = np.random.default_rng(seed)
    flat = np.array([[0, 1], [0, 2], [0, 0], [1, 2], [1, 0], [3, 1], [0, 1]], np.int64)   # node 2 receives nothing
    rel = np.array([0, 2, 2, 1, -1, r, 0], np.int64)                                       # two ids out of range
    p = {key: rng.normal(size=shape) for key, shape in (("w0", (k, u)), ("b0", (u,)), ("kernel", (r, k, u)),
                                                         ("bias", (u,)), ("wg", (r, k, u)), ("bg", (u,)),
                                                         ("wt", (r, k, u)), ("bt", (u,)))}
    return flat, rel, rng.normal(size=(4, k)), rng.normal(size=(len(flat), 1)), p


def _np_act(name, x):
    return {"linear": x, "relu": np.maximum(x, 0), "swish": x / (1 + np.exp(-x)), "sigmoid": 1 / (1 + np.exp(-x)),
            "tanh": np.tanh(x)}[name]


def test_blocks_against_a_per_edge_loop():
    flat, rel, n, w, p = _tiny()
    r = p["kernel"].shape[0]
    kern = lambda name, q: p[name][q] if 0 <= q < r else np.zeros_like(p[name][0])
    h_rgcn, h_film = np.zeros((4, 4)), np.zeros((4, 4))
    for e, (i, j) in enumerate(flat):
        msg = n[j] @ kern("kernel", rel[e]) + p["bias"]
        h_rgcn[i] += w[e, 0] * msg
        gamma = _np_act("sigmoid", n[i] @ kern("wg", rel[e]) + p["bg"])
        beta = _np_act("sigmoid", n[i] @ kern("wt", rel[e]) + p["bt"])
        h_film[i] += gamma * msg + beta
    want_rgcn = _np_act("swish", h_rgcn + _np_act("relu", n @ p["w0"] + p["b0"]))
    want_film = _np_act("tanh", h_film)
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    pt = {key: t(v) for key, v in p.items()}
    got = ref.rgcn_block(t(n), flat, t(w), rel, pt, "relu", "swish").numpy()
    assert np.max(np.abs(got - want_rgcn)) <= 1e-13
    assert np.allclose(got[2], _np_act("swish", _np_act("relu", n[2] @ p["w0"] + p["b0"])), rtol=0, atol=1e-14)
    got = ref.film_block(t(n), flat, rel, pt, "sigmoid", "tanh").numpy()
    assert np.max(np.abs(got - want_film)) <= 1e-13 and np.all(got[2] == 0.0)


def test_the_fused_identity_in_float64():
    """What csrc/mp_rgcn.hip computes - the edge sum in front of the per-relation product, zero kernels for ids out of
    range - equals the per-edge restatement to rounding."""
    flat, rel, n, w, p = _tiny(seed=8)
    r, u = p["kernel"].shape[0], p["kernel"].shape[2]
    h_rgcn, h_film = np.zeros((4, u)), np.zeros((4, u))
    for i in range(4):
        mine = [e for e in range(len(flat)) if flat[e, 0] == i]
        h_rgcn[i] = sum(w[e, 0] for e in mine) * p["bias"]
        for q in range(r):
            es = [e for e in mine if rel[e] == q]
            if not es:
                continue
            h_rgcn[i] += sum(w[e, 0] * n[flat[e, 1]] for e in es) @ p["kernel"][q]
            gamma = _np_act("sigmoid", n[i] @ p["wg"][q] + p["bg"])
            beta = _np_act("sigmoid", n[i] @ p["wt"][q] + p["bt"])
            h_film[i] += gamma * (sum(n[flat[e, 1]] for e in es) @ p["kernel"][q] + len(es) * p["bias"]) + len(es) * beta
        outside = sum(1 for e in mine if not 0 <= rel[e] < r)
        h_film[i] += outside * (p["bias"] * _np_act("sigmoid", p["bg"]) + _np_act("sigmoid", p["bt"]))
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    pt = {key: t(v) for key, v in p.items()}
    want = ref.rgcn_block(t(n), flat, t(w), rel, pt, "linear", "swish").numpy()
    assert np.max(np.abs(_np_act("swish", h_rgcn + n @ p["w0"] + p["b0"]) - want)) <= 1e-13
    want = ref.film_block(t(n), flat, rel, pt, "sigmoid", "swish").numpy()
    assert np.max(np.abs(_np_act("swish", h_film) - want)) <= 1e-13


def test_effective_kernel_restatement():
    rng = np.random.default_rng(2)
    kernel, lin = rng.normal(size=(3, 2, 4, 5)), rng.normal(size=(6, 3))
    full = np.zeros((3, 8, 10))
    for b in range(3):
        for i in range(2):
            full[b, 4 * i:4 * i + 4, 5 * i:5 * i + 5] = kernel[b, i]
    want = np.einsum("rb,bku->rku", lin, full)
    got = ref.effective_kernel(torch.tensor(kernel), torch.tensor(lin), 2).numpy()
    assert got.shape == (6, 8, 10) and np.max(np.abs(got - want)) <= 1e-14
    assert np.array_equal(ref.effective_kernel(torch.tensor(kernel), None, 2).numpy(), full)


def test_kernel_cases_deliver_their_shapes():
    """The index lists of the GPU kernel cases: the hub degrees inside one 16-receiver tile, isolated receivers, empty
    graphs, a tile of more than 256 positions, every relation pattern the names promise."""
    import topologies as topo
    cases = {name: ref.kernel_case(**kw) for name, kw in ref.kernel_cases().items()}
    assert sorted({c["rows"] for c in cases.values()}) == [1, 15, 16, 17, 20, 33]
    assert {c["r"] for c in cases.values()} == {1, 3, 20, 64}
    assert {(c["k"], c["u"]) for c in cases.values()} == {(64, 64), (32, 128), (128, 32)}
    for name in ("n15-sorted-r1", "n16-shuffled-r64", "n17-sorted-r20"):
        c = cases[name]
        deg = topo.in_degrees(c["flat"], c["rows"])
        assert sorted(deg[deg > 0]) == [1, 7, 31, 32, 33, 100] and np.all(np.nonzero(deg)[0] < 16) and (deg == 0).any()
        assert np.any(c["flat"][:, 0] == c["flat"][:, 1])                      # self loops
    c = cases["n17-sorted-r20"]
    assert 5 not in set(c["rel"]) and len(set(c["rel"])) == 19 and np.all(np.diff(c["flat"][:, 0]) >= 0)
    assert np.any(c["edge_weights"] < 0) and np.any(c["edge_weights"] == 0)
    c = cases["n33-shuffled-r64-empty-graphs"]
    assert len(c["row_splits"]) == 6 and list(np.diff(c["row_splits"])) == [0, 17, 0, 16, 0]
    ring = c["rel"][c["index_splits"][3]:c["index_splits"][4]]
    assert len(ring) == 32 and (set(ring) - {-1, 64}) <= set(range(32)) and -1 in c["rel"] and 64 in c["rel"]
    assert not np.all(np.diff(c["flat"][:, 0]) >= 0)
    assert set(cases["n33-sorted-r20-one-relation"]["rel"]) == {19}
    assert len(cases["n16-shuffled-r64"]["flat"]) == 204 and len(set(cases["n16-shuffled-r64"]["rel"])) == 64
    assert len(cases["n1-e0"]["flat"]) == 0 and len(cases["n17-e0"]["flat"]) == 0
    assert np.all(cases["n1-self-loops-r3"]["flat"] == 0) and len(cases["n1-self-loops-r3"]["flat"]) == 3
    deg = topo.in_degrees(cases["chunks-sorted-r20-oor"]["flat"], 20)
    assert list(deg[:5]) == [100, 0, 157, 3, 300] and deg[:16].sum() == 560
    for c in cases.values():
        if c["params"]["bias"] is None:
            assert c["params"]["b0"] is None and c["params"]["bg"] is None


@pytest.mark.parametrize("kind", ["rgcn", "film"])
def test_float32_restatement_noise_floor(kind):
    """Under the test weights the float32 restatement of the model cases the GPU tests run stays within 5e-6
    (rowwise_rel) of its float64 twin - the condition under which float32 pipelines are compared at parity.py's bars."""
    for name, (kw, fwd, seed) in ref.model_cases(kind).items():
        make = RGCN.make_model if kind == "rgcn" else GNNFilm.make_model
        model = make(**kw)
        ws, b = ref.parity_weights(model, seed), ref.model_batch(fwd["embed"], seed)
        r32, r64 = (ref.model_forward(kind, ws, b, dt, **fwd).numpy() for dt in (torch.float32, torch.float64))
        err = rowwise_rel(r32, r64)
        print("[noise floor] %s %s: %.2e (scale %.3g)" % (kind, name, err, float(np.max(np.abs(r64)))))
        assert err <= 5e-6, (name, err)
