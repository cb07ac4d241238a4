"""DimeNet++ API on the CPU: builder and layer configs against the reference's keys, the host Bessel tables against the
fixture, ``synth.angle_pairs`` against the reference's known answers, the torch restatement against the reference asset
and the guards."""
import os

import numpy as np
import pytest
import torch

import dimenet_reference as ref
from gcnn_keras_amd import _ffi, synth
from gcnn_keras_amd.layers.base import Layer
from gcnn_keras_amd.layers.conv.dimenet_conv import (DimNetInteractionPPBlock, DimNetOutputBlock, EmbeddingDimeBlock,
                                                     ResidualLayer, SphericalBasisLayer,
                                                     spherical_bessel_jn_normalization_prefactor,
                                                     spherical_bessel_jn_zeros)
from gcnn_keras_amd.layers.geom import EdgeAngle, VectorAngle
from gcnn_keras_amd.literature import DimeNetPP


def _fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "spherical_basis_reference.npz"))


def test_model_default_and_builder():
    assert DimeNetPP.model_default["num_spherical"] == 7 and DimeNetPP.model_default["num_radial"] == 6
    assert DimeNetPP.model_default["int_emb_size"] == 64 and DimeNetPP.model_default["basis_emb_size"] == 8
    assert DimeNetPP.__model_version__ == "2022.11.25"
    m = DimeNetPP.make_model(**synth.DIMENET_MD17)
    assert m.auto_graph is True
    names = [type(layer).__name__ for layer in m.layers]
    assert names.count("DimNetInteractionPPBlock") == 4 and names.count("DimNetOutputBlock") == 5
    shapes = [tuple(t.shape) for _, t in m.weights]
    assert shapes[0] == (96, 128)                     # EmbeddingDimeBlock: (input_dim + 1, output_dim)
    assert (42, 8) in shapes and (8, 64) in shapes    # W_sbf1, W_sbf2
    with pytest.raises(ValueError):
        DimeNetPP.make_model(output_embedding="node")
    with pytest.raises(ValueError):
        DimeNetPP.make_model(unknown_key=1)
    with pytest.raises(NotImplementedError, match="make_model"):
        DimeNetPP.make_crystal_model()


def test_layer_configs_match_reference_keys():
    base = {"name", "trainable", "dtype", "node_indexing", "ragged_validate", "is_sorted", "has_unconnected"}
    sbf = SphericalBasisLayer(7, 6, 5.0)
    assert set(sbf.get_config()) == base | {"num_radial", "cutoff", "envelope_exponent", "num_spherical"}
    dense_keys = {"kernel_regularizer", "activity_regularizer", "bias_regularizer", "kernel_constraint",
                  "bias_constraint", "kernel_initializer", "bias_initializer", "activation"}
    res = ResidualLayer(16)
    assert set(res.get_config()) == base | dense_keys | {"use_bias", "units"}
    blk = DimNetInteractionPPBlock(128, 64, 8, 1, 2)
    assert set(blk.get_config()) == base | dense_keys | {"use_bias", "pooling_method", "emb_size", "int_emb_size",
                                                         "basis_emb_size", "num_before_skip", "num_after_skip"}
    assert blk.get_config()["kernel_initializer"] == "kgcnn>glorot_orthogonal"
    assert blk.get_config()["activation"] == "kgcnn>swish"
    out = DimNetOutputBlock(128, 256, 3, num_targets=1)
    assert set(out.get_config()) == base | dense_keys | {"output_kernel_initializer", "pooling_method", "use_bias",
                                                         "emb_size", "out_emb_size", "num_dense", "num_targets"}
    emb = EmbeddingDimeBlock(95, 128)
    assert set(emb.get_config()) == {"name", "trainable", "dtype", "input_dim", "output_dim",
                                     "embeddings_initializer", "embeddings_regularizer", "embeddings_constraint"}
    assert tuple(emb.embeddings.shape) == (96, 128)
    assert EdgeAngle(vector_scale=[1.0, -1.0]).get_config()["vector_scale"] == [1.0, -1.0]
    assert "vector_scale" not in VectorAngle().get_config()
    assert DimNetInteractionPPBlock(128, 64, 8, 1, 2).fused_triplet(42)
    assert not DimNetInteractionPPBlock(128, 32, 8, 1, 2).fused_triplet(42)
    assert not DimNetInteractionPPBlock(128, 64, 8, 1, 2).fused_triplet(100)


def test_abi_symbols_declared():
    names = set(_ffi.declared_symbols())
    for n in ("mp_vector_angle_f32", "mp_vector_angle_grad_f32", "mp_edge_angle_f32", "mp_edge_angle_grad_ws_bytes",
              "mp_edge_angle_grad_f32", "mp_spherical_basis_f32", "mp_spherical_basis_grad_f32",
              "mp_dimenet_triplet_f32", "mp_dimenet_triplet_grad_f32"):
        assert n in names
    header = _ffi.HEADER_TEXT
    assert "int mp_dimenet_triplet_f32(" in header and "#define MP_SBF_MAX_RADIAL 64" in header


@pytest.mark.parametrize("size", [(7, 6), (10, 10)])
def test_host_tables_match_fixture(golden_dir, size):
    f = _fixture(golden_dir)
    z = spherical_bessel_jn_zeros(*size)
    assert z.dtype == np.float32
    np.testing.assert_allclose(z, f["zeros_%d_%d" % size], rtol=1e-6)
    nrm = spherical_bessel_jn_normalization_prefactor(*size)
    np.testing.assert_allclose(nrm, f["norm_%d_%d" % size], rtol=1e-6)
    layer = SphericalBasisLayer(size[0], size[1], 5.0)
    tab = layer.host_tables()
    lr = size[0] * size[1]
    assert tab.dtype == np.float32 and tab.size == 2 * lr + size[0] * (size[0] // 2 + 1) + size[0]
    np.testing.assert_array_equal(tab[:lr], z.ravel())


def test_angle_pairs_known_answers(golden_dir):
    # kgcnn test/test_adj.py:47-68: the triples (i, j, k) of the pairs n = (i, j), m = (j, k), and the matching rule
    def triples(idx):
        pairs = synth.angle_pairs(idx)
        return np.concatenate([idx[pairs[:, 0]], idx[pairs[:, 1]][:, 1:]], axis=-1)

    edi1 = np.array([[0, 1], [0, 2], [1, 0], [1, 2], [2, 0], [2, 1]])
    edi2 = np.array([[0, 1], [0, 2], [1, 0], [2, 0]])
    np.testing.assert_array_equal(triples(edi2), [[1, 0, 2], [2, 0, 1]])
    np.testing.assert_array_equal(triples(edi1), [[0, 1, 2], [0, 2, 1], [1, 0, 2], [1, 2, 0], [2, 0, 1], [2, 1, 0]])
    edi = np.array([[0, 1], [1, 0], [1, 6], [2, 3], [3, 2], [3, 5], [3, 7], [4, 7], [5, 3], [6, 1], [6, 7],
                    [7, 3], [7, 4], [7, 6]])
    nm = synth.angle_pairs(edi)
    assert len(nm) and np.all(edi[nm[:, 0]][:, 1] == edi[nm[:, 1]][:, 0])
    g = np.load(os.path.join(golden_dir, "bessel_basis_reference.npz"))
    f = _fixture(golden_dir)
    np.testing.assert_array_equal(synth.angle_pairs(g["ei0"]), f["angles_0"])
    np.testing.assert_array_equal(synth.angle_pairs(g["ei1"]), f["angles_1"])
    assert len(f["angles_1"]) == 954
    assert synth.angle_pairs(np.zeros((0, 2), np.int64)).shape == (0, 2)


def test_dimenet_batch_and_params():
    b = synth.dimenet_batch(num_graphs=3, seed=1)
    assert b["angle_splits"][-1] == len(b["angle_indices"])
    es = b["edge_splits"]
    for g in range(3):
        a = b["angle_indices"][b["angle_splits"][g]:b["angle_splits"][g + 1]]
        assert a.min() >= 0 and a.max() < es[g + 1] - es[g]
    m = DimeNetPP.make_model(**synth.DIMENET_MD17)
    p = synth.dimenet_params(m, seed=2)
    assert [v.shape for v in p.values()] == [tuple(t.shape) for _, t in m.weights]
    finals = [v for k, v in p.items() if "dense_final" in k or k.endswith("kernel") and v.shape[-1] == 1]
    assert finals and all(np.any(v != 0) for v in finals)


def test_restatement_matches_reference_asset(golden_dir):
    f = _fixture(golden_dir)
    g = np.load(os.path.join(golden_dir, "bessel_basis_reference.npz"))
    layer = SphericalBasisLayer(10, 10, 5.0)
    for dtype in (torch.float64, torch.float32):
        for x, ei, a, want, rows in ((g["x0"], g["ei0"], f["angles_0"], f["spherical_basis_0"], None),
                                     (g["x1"], g["ei1"], f["angles_1"], f["spherical_basis_1_rows"], f["rows_1"])):
            xt = torch.tensor(x, dtype=dtype)
            ei_t, a_t = torch.from_numpy(ei), torch.from_numpy(a)
            v = xt[ei_t[:, 0]] - xt[ei_t[:, 1]]
            d = torch.linalg.norm(v, dim=-1)
            th = ref.vector_angle(v[a_t[:, 0]], v[a_t[:, 1]])
            s = ref.spherical_basis(d, th, a_t[:, 1], layer, dtype).numpy()
            s = s if rows is None else s[rows]
            assert np.max(np.abs(s - want)) < 0.05         # the reference's own bar (test_geom.py:75-76)


def test_restatement_forces_match_finite_differences():
    b = synth.dimenet_batch(num_graphs=2, seed=4, min_distance=0.9, sizes=[5, 7])
    m = DimeNetPP.make_model(**dict(synth.DIMENET_MD17, num_blocks=1, emb_size=16, out_emb_size=16))
    p = list(synth.dimenet_params(m, seed=5).values())
    _, force = ref.energy_forces(p, b, m)
    x0 = torch.tensor(b["node_coordinates"], dtype=torch.float64)
    h = 1e-6
    for atom, comp in ((0, 0), (3, 2), (6, 1), (10, 0)):
        xp, xm = x0.clone(), x0.clone()
        xp[atom, comp] += h
        xm[atom, comp] -= h
        ep = ref.dimenet_forward(p, b, m, xyz=xp).sum()
        em = ref.dimenet_forward(p, b, m, xyz=xm).sum()
        fd = -(ep - em).item() / (2 * h)
        assert abs(fd - force[atom, comp].item()) <= 1e-6 * max(1.0, abs(fd))


def test_guards():
    with pytest.raises(AssertionError):
        SphericalBasisLayer(7, 65, 5.0)
    with pytest.raises(ValueError):
        SphericalBasisLayer(_ffi.MP_SBF_MAX_SPHERICAL + 1, 6, 5.0)
    with pytest.raises(ValueError):
        SphericalBasisLayer(7, 6, 0.0)
    with pytest.raises(AssertionError):
        EdgeAngle(vector_scale=[1.0])
    assert _ffi.activation_code("kgcnn>swish") == _ffi.activation_code("swish")
    w = Layer().add_weight("w", (4, 6), "kgcnn>glorot_orthogonal", device="cpu")
    assert abs(float(w.var(unbiased=False)) - 1.0 / 5.0) < 1e-5
    u = Layer().add_weight("u", (50, 4), {"class_name": "RandomUniform", "config": {"minval": 2.0, "maxval": 3.0}},
                           device="cpu")
    assert float(u.min()) >= 2.0 and float(u.max()) <= 3.0
    with pytest.raises(ValueError):
        Layer().add_weight("v", (2, 2), {"class_name": "TruncatedNormal", "config": {}}, device="cpu")
