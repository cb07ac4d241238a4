"""Periodic cells without a GPU: the interface of ``SetRangePeriodic`` and of the crystal builders, and the pin of
tests/periodic_reference.py (the restatement the GPU tests compare against): its neighbour sets equal the reference's
golden sets (tests/golden/periodic_cases.npz), and its crystal energies obey the super-cell and lattice-translation
identities in float64."""
import numpy as np
import pytest
import torch

import periodic_reference as pr
from gcnn_keras_amd import synth
from oracle import torch_force_oracle as tfo


# ------------------------------------------------------------------------------------------------------------- interface
def test_set_range_periodic_defaults_and_config():
    from gcnn_keras_amd.graph.preprocessor import SetRangePeriodic
    cfg = SetRangePeriodic().get_config()
    assert cfg == {"name": "set_range_periodic", "node_coordinates": "node_coordinates",
                   "range_indices": "range_indices", "graph_lattice": "graph_lattice", "range_image": "range_image",
                   "range_attributes": "range_attributes", "max_distance": 4.0, "max_neighbours": None,
                   "exclusive": True, "do_invert_distance": False, "self_loops": False, "overwrite": True}
    sp = SetRangePeriodic(range_indices="ri", range_image="im", range_attributes="ra", max_distance=5.0,
                          max_neighbours=12, overwrite=False, name="x")
    assert sp.produces == ("ri", "im", "ra")
    assert SetRangePeriodic(**sp.get_config()).get_config() == sp.get_config()


@pytest.mark.parametrize("kwargs", [{"self_loops": True}, {"exclusive": False}, {"do_invert_distance": True},
                                    {"max_distance": None}])
def test_set_range_periodic_refuses_uncovered_modes(kwargs):
    from gcnn_keras_amd.graph.preprocessor import SetRangePeriodic
    with pytest.raises(NotImplementedError):
        SetRangePeriodic(**kwargs)


def test_set_range_periodic_has_no_cpu_fallback():
    from gcnn_keras_amd import _ffi
    from gcnn_keras_amd.graph.preprocessor import SetRangePeriodic
    from gcnn_keras_amd.ragged import RaggedTensor
    xyz = RaggedTensor(torch.zeros(2, 3), torch.tensor([0, 2]))
    with pytest.raises(_ffi.EngineError):
        SetRangePeriodic()(xyz, torch.eye(3).reshape(1, 3, 3))
    with pytest.raises(ValueError):
        SetRangePeriodic()(xyz)


def test_periodic_entry_points_check_their_arguments():
    from gcnn_keras_amd import _ffi
    lib = _ffi.lib()
    assert lib.mp_lattice_shift_f32(None, None, None, None, 0, 0, None, None) == _ffi.MP_OK
    assert lib.mp_lattice_shift_f32(None, None, None, None, 1, 4, None, None) == _ffi.MP_EINVAL
    assert lib.mp_radius_graph_periodic_fill_f32(None, None, None, 0, 0, 4.0, -1, None, 0, None, None, None, None, None,
                                                 None) == _ffi.MP_OK
    assert lib.mp_radius_graph_periodic_count_f32(None, None, None, 1, 1, 4.0, -1, None, None, None, None, 0,
                                                  None) == _ffi.MP_EINVAL
    assert b"mp_radius_graph_periodic_count_f32" in lib.mp_last_error()


def test_schnet_crystal_builder():
    from gcnn_keras_amd.literature import Schnet
    d = Schnet.model_crystal_default
    assert [i["name"] for i in d["inputs"]] == ["node_number", "node_coordinates", "edge_indices", "edge_image",
                                                "graph_lattice"]
    assert d["inputs"][4] == {"shape": (3, 3), "name": "graph_lattice", "dtype": "float32", "ragged": False}
    assert {k: v for k, v in d.items() if k != "inputs"} == {k: v for k, v in Schnet.model_default.items()
                                                             if k != "inputs"}
    # decorated with the molecular defaults, as in the reference: without inputs it sees three and says what to pass
    with pytest.raises(ValueError, match=r'model_crystal_default\["inputs"\]'):
        Schnet.make_crystal_model()
    with pytest.raises(ValueError, match=r'model_crystal_default\["inputs"\]'):
        Schnet.make_crystal_model(inputs=d["inputs"][:4])
    with pytest.raises(ValueError):
        Schnet.make_crystal_model(inputs=d["inputs"], output_embedding="edge")
    with pytest.raises(ValueError):
        Schnet.make_crystal_model(inputs=d["inputs"], no_such_option=1)
    crystal = Schnet.make_crystal_model(inputs=d["inputs"], depth=2)
    mol = Schnet.make_model(depth=2)
    assert [(n.split("/")[-1], tuple(t.shape)) for n, t in crystal.weights] == \
        [(n.split("/")[-1], tuple(t.shape)) for n, t in mol.weights]   # same layers in the same order
    assert crystal.fused is None and crystal.auto_graph is True
    assert mol.auto_graph is False   # the molecular builder is as it was


def test_painn_crystal_builder():
    from gcnn_keras_amd.literature import PAiNN
    d = PAiNN.model_crystal_default
    assert [i["name"] for i in d["inputs"]] == ["node_attributes", "node_coordinates", "edge_indices", "edge_image",
                                                "graph_lattice"]
    assert {k: v for k, v in d.items() if k != "inputs"} == {k: v for k, v in PAiNN.model_default.items()
                                                             if k != "inputs"}
    with pytest.raises(ValueError, match=r'model_crystal_default\["inputs"\]'):
        PAiNN.make_crystal_model(inputs=d["inputs"][:3])
    for refused in ({"equiv_normalization": True}, {"node_normalization": True}):
        with pytest.raises(NotImplementedError):
            PAiNN.make_crystal_model(**refused)
    with pytest.raises(ValueError):
        PAiNN.make_crystal_model(output_embedding="edge")
    crystal = PAiNN.make_crystal_model(depth=2)      # decorated with the crystal defaults: five inputs without asking
    mol = PAiNN.make_model(depth=2)
    assert [(n.split("/")[-1], tuple(t.shape)) for n, t in crystal.weights] == \
        [(n.split("/")[-1], tuple(t.shape)) for n, t in mol.weights]   # same layers in the same order
    assert crystal.fused is None and crystal.auto_graph is True
    assert mol.fused is not None and mol.auto_graph is False


def test_dimenet_crystal_model_still_raises():
    from gcnn_keras_amd.literature import DimeNetPP
    with pytest.raises(NotImplementedError):
        DimeNetPP.make_crystal_model()


# ------------------------------------------------------------------------------------------------ the restatement, pinned
@pytest.fixture(scope="module")
def cases(golden_dir):
    return pr.golden_cases(golden_dir)


NAMES = ["cubic1_c40", "tri5_c40", "tri5_c46", "tri5_c55", "tri5_c40_n12", "unwrapped_c40", "thin2_c40", "big6_c40"]


def test_golden_holds_the_cases_of_the_issue(cases):
    assert list(cases) == NAMES
    assert len(cases["cubic1_c40"]["indices"]) == 6
    assert len(cases["unwrapped_c40"]["indices"]) == len(cases["tri5_c40"]["indices"])
    assert np.abs(cases["unwrapped_c40"]["images"]).max() >= 3
    deg = lambda c: np.bincount(cases[c]["indices"][:, 0], minlength=len(cases[c]["xyz"]))
    assert deg("tri5_c40").max() < 64 < deg("tri5_c46").min() and deg("tri5_c46").max() < 128 < deg("tri5_c55").max()
    assert deg("big6_c40").min() == 0 and np.all(deg("tri5_c40_n12") == 12)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restated_neighbour_rule_equals_the_reference(cases, name, dtype):
    c = cases[name]
    idx, img, d = pr.neighbours(c["xyz"], c["lattice"], c["cutoff"], c["maxn"], dtype)
    assert pr.edge_set(idx, img) == pr.edge_set(c["indices"], c["images"])
    assert len(idx) == len(c["indices"])
    assert np.array_equal(idx[:, 0], c["indices"][:, 0])            # receivers in node order
    for i in range(len(c["xyz"])):
        mine, ref = d[idx[:, 0] == i], c["dist"][c["indices"][:, 0] == i]
        assert np.all(np.diff(mine) >= 0)
        # sorted distances agree whatever the order inside a tie: float64 to rounding, float32 to its resolution at 5.5
        assert np.max(np.abs(mine - ref), initial=0.0) <= (1e-12 if dtype is np.float64 else 2e-6)


def test_lattice_shift_restatement_is_the_reduce_sum_order():
    rng = np.random.default_rng(5)
    pos, lat = rng.normal(size=(7, 3)).astype(np.float32), rng.normal(size=(7, 3, 3)).astype(np.float32)
    img = rng.integers(-3, 4, size=(7, 3))
    got = pr.lattice_shift_np(pos, img, lat)
    want = pos + np.sum(lat * img.astype(np.float32)[:, :, None], axis=1)   # kgcnn/layers/geom.py:119-120
    assert got.dtype == np.float32 and np.array_equal(got, want)


# Heads that are extensive (twice the atoms, twice the energy): SchNet with the per-atom energy read out in front of the
# pooling (the fork's layout), PaiNN with a linear output MLP without biases behind it.
SCHNET_P = synth.schnet_params(seed=17, depth=2, last_units=(128, 64, 1), out_units=(), random_bias=True)
PAINN_P = synth.painn_params(seed=18, depth=2, random_bias=True)
PAINN_P.update({k: np.zeros_like(v) for k, v in PAINN_P.items() if k.startswith("output_mlp") and k.endswith("bias")})
MODELS = [("schnet", SCHNET_P, {"depth": 2, "last_mlp_act": ("kgcnn>shifted_softplus",) * 2 + ("linear",),
                                "output_mlp_act": ()}),
          ("painn", PAINN_P, {"depth": 2, "equiv_method": "eps", "output_mlp_act": ("linear", "linear")})]

# Both identities compare two float64 evaluations of the same sums in another order.  Measured here, relative to the
# energy / the largest force component: super-cell SchNet 3.9e-16 / 4.1e-16, PaiNN 1.2e-15 / 3.2e-16; translation 0 / 0
# for both (coordinates and lattice are float32 numbers, so the float64 shifts are exact).  The bound is ~100 x the worst.
IDENTITY_RTOL = 1e-13


@pytest.mark.parametrize("kind,params,kw", MODELS, ids=["schnet", "painn"])
def test_super_cell_gives_twice_the_energy_and_the_same_forces(monkeypatch, cases, kind, params, kw):
    c = cases["tri5_c40"]
    xyz, lat = c["xyz"].astype(np.float64), c["lattice"].astype(np.float64)
    numbers = np.array([1, 6, 7, 8, 6])
    p = tfo.to_torch(params, torch.float64)

    def run(x, cell, z):
        idx, img, _ = pr.neighbours(x, cell, c["cutoff"])
        b = {"node_number": z, "node_splits": np.array([0, len(x)]), "edge_splits": np.array([0, len(idx)]),
             "edge_indices": idx, "edge_image": img, "graph_lattice": cell[None]}
        xt = torch.from_numpy(x).requires_grad_(True)
        e = pr.crystal_energy(monkeypatch, kind, p, b, xyz=xt, **kw)
        f, = torch.autograd.grad(e.sum(), xt)
        return e, f, len(idx)

    ea, fa, m1 = run(xyz, lat, numbers)
    eb, fb, m2 = run(np.concatenate([xyz, xyz + lat[0]]), np.stack([2.0 * lat[0], lat[1], lat[2]]),
                     np.concatenate([numbers, numbers]))
    assert m2 == 2 * m1
    err_e = abs(float(eb.detach()) - 2 * float(ea.detach())) / abs(float(ea.detach()))
    scale = float(fa.abs().max())
    err_f = max(float((fb[:5] - fa).abs().max()), float((fb[5:] - fa).abs().max())) / scale
    print("[identity] %s super-cell: energy %.2e, forces %.2e" % (kind, err_e, err_f))
    assert err_e <= IDENTITY_RTOL and err_f <= IDENTITY_RTOL


@pytest.mark.parametrize("kind,params,kw", MODELS, ids=["schnet", "painn"])
def test_moving_an_atom_by_a_lattice_vector_changes_nothing(monkeypatch, cases, kind, params, kw):
    c = cases["tri5_c40"]
    xyz, lat = c["xyz"].astype(np.float64), c["lattice"].astype(np.float64)
    numbers = np.array([1, 6, 7, 8, 6])
    moved = xyz.copy()
    moved[2] += 2.0 * lat[0] - lat[1]
    p = tfo.to_torch(params, torch.float64)
    out = []
    for x in (xyz, moved):
        idx, img, _ = pr.neighbours(x, lat, c["cutoff"])
        b = {"node_number": numbers, "node_splits": np.array([0, 5]), "edge_splits": np.array([0, len(idx)]),
             "edge_indices": idx, "edge_image": img, "graph_lattice": lat[None]}
        xt = torch.from_numpy(x).requires_grad_(True)
        e = pr.crystal_energy(monkeypatch, kind, p, b, xyz=xt, **kw)
        f, = torch.autograd.grad(e.sum(), xt)
        out.append((float(e.detach()), f.numpy(), pr.edge_set(idx, img)))
    assert out[0][2] != out[1][2] and len(out[0][2]) == len(out[1][2])     # the images were re-derived
    err_e = abs(out[1][0] - out[0][0]) / abs(out[0][0])
    err_f = float(np.max(np.abs(out[1][1] - out[0][1]))) / float(np.max(np.abs(out[0][1])))
    print("[identity] %s translation: energy %.2e, forces %.2e" % (kind, err_e, err_f))
    assert err_e <= IDENTITY_RTOL and err_f <= IDENTITY_RTOL
