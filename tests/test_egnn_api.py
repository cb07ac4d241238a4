"""EGNN API on the CPU: builder defaults and weight shapes against the reference's, the two quirks of the reference's
builder, layer configs, guards, the host frequency table, and the torch restatement (tests/egnn_reference.py) against
finite differences and the model's symmetries."""
import numpy as np
import pytest
import torch

import egnn_reference as ref
from gcnn_keras_amd import _ffi, synth
from gcnn_keras_amd.layers.conv.egnn_conv import FUSED_EDGE_SIZES
from gcnn_keras_amd.layers.geom import PositionEncodingBasisLayer, position_encoding_scales
from gcnn_keras_amd.literature import EGNN

# kgcnn/literature/EGNN.py:23-53
REFERENCE_KEYS = ["name", "inputs", "input_embedding", "depth", "node_mlp_initialize", "euclidean_norm_kwargs",
                  "use_edge_attributes", "edge_mlp_kwargs", "edge_attention_kwargs", "use_normalized_difference",
                  "expand_distance_kwargs", "coord_mlp_kwargs", "pooling_coord_kwargs", "pooling_edge_kwargs",
                  "node_normalize_kwargs", "use_node_attributes", "node_mlp_kwargs", "use_skip", "verbose",
                  "node_decoder_kwargs", "node_pooling_kwargs", "output_embedding", "output_to_tensor", "output_mlp"]


def _shapes(m):
    return [tuple(t.shape) for _, t in m.weights]


def test_model_default_keys_and_values():
    d = EGNN.model_default
    assert list(d) == REFERENCE_KEYS
    assert d["name"] == "EGNN" and d["depth"] == 4 and d["use_edge_attributes"] is True and d["use_skip"] is True
    assert d["euclidean_norm_kwargs"] == {"keepdims": True, "axis": 2}
    assert d["edge_mlp_kwargs"] == {"units": [64, 64], "activation": ["swish", "linear"]}
    assert d["coord_mlp_kwargs"] == {"units": [64, 1], "activation": ["swish", "linear"]}
    assert d["pooling_coord_kwargs"] == {"pooling_method": "mean"} and d["pooling_edge_kwargs"] == {"pooling_method": "sum"}
    assert d["edge_attention_kwargs"] is None and d["expand_distance_kwargs"] is None and d["node_decoder_kwargs"] is None
    assert d["output_mlp"] == {"use_bias": [True, True], "units": [64, 1], "activation": ["swish", "linear"]}
    assert d["inputs"][3]["shape"] == (None, 10) and d["input_embedding"]["node"] == {"input_dim": 95, "output_dim": 64}
    assert EGNN.__model_version__ == "2022.11.25"


def test_weight_shapes_md17_qm9_default():
    m = EGNN.make_model(**synth.EGNN_MD17)
    s = _shapes(m)
    assert m.auto_graph is True and m.use_fused_edge is True and m.fused_edge_blocks == [True] * 7
    assert s[:2] == [(15, 128), (128,)]                                   # node_mlp_initialize, no embeddings
    block = [(276, 128), (128,), (128, 128), (128,), (128, 1), (1,), (256, 128), (128,), (128, 128), (128,)]
    for i in range(7):
        assert s[2 + 10 * i: 12 + 10 * i] == block, i
    assert s[72:] == [(128, 128), (128,), (128, 128), (128,), (128, 128), (128,), (128, 1), (1,)]   # decoder, output MLP
    q = EGNN.make_model(**synth.EGNN_QM9)
    assert _shapes(q)[2] == (257, 128) and len(_shapes(q)) == len(s) and q.fused_edge_blocks == [True] * 7
    d = EGNN.make_model()
    sd = _shapes(d)
    assert sd[0] == (95, 64)                                              # node embedding; edge attributes are dense
    assert sd[1:9] == [(139, 64), (64,), (64, 64), (64,), (64, 64), (64,), (64, 1), (1,)]   # edge MLP, coordinate MLP
    assert sd[9:13] == [(128, 64), (64,), (64, 64), (64,)] and len(sd) == 1 + 4 * 12 + 4
    assert d.fused_edge_blocks == [False] * 4                             # width 64, edge attributes, coordinate model
    arrays = m.get_weights()
    m.set_weights(arrays)
    assert all(a.shape == b for a, b in zip(arrays, s))


def test_the_two_quirks_of_the_reference_builder():
    # expand_distance_kwargs only switches the encoding on: dim_half 64 still gives 20 columns (EGNN.py:151-152)
    m = EGNN.make_model(**synth.EGNN_MD17)
    enc = [lay for lay in m.layers if isinstance(lay, PositionEncodingBasisLayer)]
    assert len(enc) == 7 and all(e.dim_half == 10 and e.num_mult == 100 and e.wave_length_min == 1 for e in enc)
    assert _shapes(m)[2][0] == 2 * 128 + 20
    # the decoder is built from node_mlp_kwargs (EGNN.py:188-189)
    cfg = dict(synth.EGNN_MD17, node_decoder_kwargs={"units": [7, 5], "activation": ["relu", "relu"]})
    s = _shapes(EGNN.make_model(**cfg))
    assert s[72:76] == [(128, 128), (128,), (128, 128), (128,)]
    assert len(_shapes(EGNN.make_model(**dict(synth.EGNN_MD17, node_decoder_kwargs=None)))) == len(s) - 4


def test_fused_route_is_chosen_from_the_configuration():
    assert FUSED_EDGE_SIZES == {"units": 128, "max_encoding": 64}
    base = synth.EGNN_MD17
    assert EGNN.make_model(**dict(base, edge_attention_kwargs=None)).fused_edge_blocks == [True] * 7
    three = {"units": [128, 128, 128], "activation": "swish"}
    assert EGNN.make_model(**dict(base, edge_mlp_kwargs=three)).fused_edge_blocks == [False] * 7
    narrow = {"units": [64, 128], "activation": "swish"}
    assert EGNN.make_model(**dict(base, edge_mlp_kwargs=narrow)).fused_edge_blocks == [False] * 7
    assert EGNN.make_model(**dict(base, pooling_edge_kwargs={"pooling_method": "mean"})).fused_edge_blocks == [False] * 7
    coord = dict(base, coord_mlp_kwargs={"units": [128, 1], "activation": ["swish", "linear"]},
                 pooling_coord_kwargs={"pooling_method": "mean"})
    assert EGNN.make_model(**coord).fused_edge_blocks == [False] * 7
    attrs = dict(base, use_edge_attributes=True)
    attrs["inputs"] = base["inputs"][:3] + [{"shape": [None, 4], "name": "e", "dtype": "float32", "ragged": True}]
    assert EGNN.make_model(**attrs).fused_edge_blocks == [False] * 7
    init64 = dict(base, node_mlp_initialize={"units": 64, "activation": "linear"},
                  node_mlp_kwargs={"units": [64, 64], "activation": ["swish", "linear"]})
    assert EGNN.make_model(**init64).fused_edge_blocks == [False] * 7


def test_guards():
    with pytest.raises(ValueError):
        EGNN.make_model(output_embedding="edge")
    with pytest.raises(ValueError):
        EGNN.make_model(unknown_key=1)
    with pytest.raises(NotImplementedError, match="GraphLayerNormalization"):
        EGNN.make_model(node_normalize_kwargs={"axis": -1})
    m = EGNN.make_model(**synth.EGNN_MD17)
    cfg = m.config
    assert cfg["expand_distance_kwargs"] == {"dim_half": 64} and cfg["depth"] == 7
    again = EGNN.make_model(name="EGNNEnergy", verbose=10, **cfg)
    assert _shapes(again) == _shapes(m)


def test_position_encoding_layer_config_and_guards():
    base = {"name", "trainable", "dtype", "node_indexing", "ragged_validate", "is_sorted", "has_unconnected"}
    lay = PositionEncodingBasisLayer()
    conf = lay.get_config()
    assert set(conf) == base | {"dim_half", "wave_length_min", "num_mult", "include_frequencies", "interleave_sin_cos"}
    assert (conf["dim_half"], conf["wave_length_min"], conf["num_mult"]) == (10, 1, 100)
    assert conf["include_frequencies"] is False and conf["interleave_sin_cos"] is False
    conf.pop("name")
    twin = PositionEncodingBasisLayer.from_config(conf)
    assert twin.get_config()["dim_half"] == 10 and lay.weights == [] and lay.weight_gradients is True
    assert PositionEncodingBasisLayer(dim_half=4, interleave_sin_cos=True).get_config()["interleave_sin_cos"] is True
    with pytest.raises(ValueError, match="num_mult"):
        PositionEncodingBasisLayer(num_mult=1)
    with pytest.raises(ValueError, match="dim_half"):
        PositionEncodingBasisLayer(dim_half=1)
    with pytest.raises(NotImplementedError):
        PositionEncodingBasisLayer(include_frequencies=True)
    s = position_encoding_scales(10, 1, 100)
    assert s.dtype == np.float32 and s.shape == (10,)
    np.testing.assert_array_equal(s, ref.encoding_scales())
    np.testing.assert_allclose(s, 2 * np.pi * 100.0 ** (-np.arange(10) / 9.0), rtol=1e-6)
    assert s[0] == np.float32(2 * np.pi)
    if not torch.cuda.is_available():
        with pytest.raises(_ffi.EngineError):           # no CPU fallback
            from gcnn_keras_amd.ragged import RaggedTensor
            lay(RaggedTensor(torch.ones(3, 1), torch.tensor([0, 3])))


def test_synth_batch_and_attributes():
    b = synth.egnn_batch(num_graphs=3, seed=1)
    assert b["node_attributes"].shape == (63, 15) and b["node_attributes"].dtype == np.float32
    assert len(b["edge_indices"]) == 3 * 420 and list(b["edge_splits"]) == [0, 420, 840, 1260]   # fully connected at 10 A
    a = synth.atomic_charge_representation(np.array([1, 6, 8, 9]))
    assert a.shape == (4, 15)
    np.testing.assert_allclose(a[1, 3:6], [1.0, 6 / 9.0, (6 / 9.0) ** 2], rtol=1e-6)
    assert np.count_nonzero(a[1]) == 3 and np.count_nonzero(a[0, :3]) == 3 and a[3, 12] == 1.0
    small = synth.egnn_batch(sizes=[1, 0, 3], max_distance=10.0)
    assert list(small["node_splits"]) == [0, 1, 1, 4] and list(small["edge_splits"]) == [0, 0, 0, 6]


# ------------------------------------------------------------------------------------------------ the restatement
SMALL = dict(synth.EGNN_MD17, depth=2, node_mlp_initialize={"units": 16, "activation": "linear"},
             edge_mlp_kwargs={"units": [16, 16], "activation": ["swish", "swish"]},
             node_mlp_kwargs={"units": [16, 16], "activation": ["swish", "linear"]},
             output_mlp={"use_bias": [True, True], "units": [16, 1], "activation": ["swish", "linear"]})
SMALL_DEFAULT = dict(depth=2)


def _small(cfg, sizes=(5, 1, 7), with_attributes=False, seed=3):
    m = EGNN.make_model(**cfg)
    w = list(synth.egnn_params(m, seed=5).values())
    b = synth.egnn_batch(sizes=list(sizes), seed=seed, min_distance=0.9, max_distance=4.0)
    if with_attributes:
        b["edge_attributes"] = np.random.default_rng(9).normal(size=(len(b["edge_indices"]), 10)).astype(np.float32)
    return m, w, b


def _rotation(seed=4):
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q * np.sign(np.linalg.det(q))


@pytest.mark.parametrize("which", ["md17-like", "default"])
def test_restatement_forces_match_finite_differences(which):
    m, w, b = _small(SMALL if which == "md17-like" else SMALL_DEFAULT, with_attributes=which == "default")
    e, f = ref.energy_forces(w, b, m.config)
    assert tuple(e.shape) == (3, 1) and tuple(f.shape) == (13, 3) and float(f.abs().max()) > 0
    x0 = torch.tensor(b["node_coordinates"], dtype=torch.float64)
    step = 1e-5
    worst = 0.0
    for atom in (0, 4, 5, 9):
        for axis in range(3):
            xp, xm = x0.clone(), x0.clone()
            xp[atom, axis] += step
            xm[atom, axis] -= step
            fd = -(ref.egnn_forward(w, b, m.config, xyz=xp).sum() - ref.egnn_forward(w, b, m.config, xyz=xm).sum()) \
                / (2 * step)
            worst = max(worst, abs(float(fd) - float(f[atom, axis])))
    assert worst <= 1e-7 * max(1.0, float(f.abs().max())), worst
    # forces of every molecule sum to zero (translation invariance), the lone atom feels none
    assert float(f[:5].sum(0).abs().max()) < 1e-10 and float(f[5].abs().max()) == 0.0


@pytest.mark.parametrize("which", ["md17-like", "default"])
def test_restatement_energy_is_invariant_and_coordinates_equivariant(which):
    m, w, b = _small(SMALL if which == "md17-like" else SMALL_DEFAULT, with_attributes=which == "default")
    rot = torch.tensor(_rotation(), dtype=torch.float64)
    shift = torch.tensor([0.3, -1.1, 2.0], dtype=torch.float64)
    x0 = torch.tensor(b["node_coordinates"], dtype=torch.float64)
    x1 = x0 @ rot.T + shift
    e0, e1 = ref.egnn_forward(w, b, m.config, xyz=x0), ref.egnn_forward(w, b, m.config, xyz=x1)
    assert float((e0 - e1).abs().max()) <= 1e-10 * max(1.0, float(e0.abs().max()))
    if which == "default":
        y0 = ref.egnn_forward(w, b, m.config, xyz=x0, return_coordinates=True)
        y1 = ref.egnn_forward(w, b, m.config, xyz=x1, return_coordinates=True)
        assert float((y0 - x0).abs().max()) > 1e-3            # the coordinate model moves the atoms
        assert float((y1 - (y0 @ rot.T + shift)).abs().max()) <= 1e-10 * max(1.0, float(y0.abs().max()))


def test_restatement_node_output_and_float32_twin():
    cfg = dict(SMALL, output_embedding="node")
    m, w, b = _small(cfg)
    out64 = ref.egnn_forward(w, b, m.config)
    out32 = ref.egnn_forward(w, b, m.config, dtype=torch.float32)
    assert tuple(out64.shape) == (13, 1) and out32.dtype == torch.float32
    assert float((out64 - out32.double()).abs().max()) <= 1e-4 * float(out64.abs().max())
    x = torch.tensor([[0.5], [2.25], [100.0]], dtype=torch.float64)
    plain, inter = ref.position_encoding(x, torch.float64), ref.position_encoding(x, torch.float64, interleave=True)
    assert tuple(plain.shape) == (3, 20)
    assert torch.equal(inter[:, 0::2], plain[:, :10]) and torch.equal(inter[:, 1::2], plain[:, 10:])
