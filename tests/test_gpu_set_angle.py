"""On-GPU ``SetAngle`` (csrc/mp_angle.hip): angle triples, edge pairs and angle values of ragged batches against the
reference's ``get_angle_indices`` output (tests/golden/angle_cases.npz), the brute-force restatement of the rule
(tests/test_set_angle_api.py::angle_rule) and the host helpers of ``gcnn_keras_amd.synth``; the attached index plans;
the MD driver running HDNNP2nd from coordinates alone.  Integers are held to ``torch.equal``."""
import functools

import numpy as np
import pytest
import torch

from gcnn_keras_amd import _ffi, synth
from gcnn_keras_amd.graph.preprocessor import SetAngle, SetRange
from gcnn_keras_amd.ragged import IndexPlan, RaggedTensor
from parity import assert_forces_close, assert_rows_close
from test_set_angle_api import NUM_CASES, PAIRINGS, angle_rule, load_cases

pytestmark = pytest.mark.gpu


def _rag(values, splits):
    return RaggedTensor.from_numpy(np.ascontiguousarray(values), np.asarray(splits, np.int64))


def _splits(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def _coordinates(node_splits, seed=0):
    xyz = np.random.default_rng(seed).normal(0.0, 1.5, size=(int(node_splits[-1]), 3)).astype(np.float32)
    return _rag(xyz, node_splits)


def _batch_of(edge_lists, node_counts):
    """Ragged ``(range_indices, node_coordinates)`` of per-graph edge lists."""
    edges = np.concatenate([np.asarray(e, np.int64).reshape(-1, 2) for e in edge_lists], axis=0)
    node_splits = _splits(node_counts)
    return _rag(edges, _splits([len(e) for e in edge_lists])), _coordinates(node_splits)


def _expect(per_graph):
    """Concatenated ``(triples, pairs, angle_splits)`` tensors of per-graph ``(triples, pairs)`` results."""
    triples = np.concatenate([t.reshape(-1, 3) for t, _ in per_graph], axis=0).astype(np.int64)
    pairs = np.concatenate([p.reshape(-1, 2) for _, p in per_graph], axis=0).astype(np.int64)
    return torch.from_numpy(triples), torch.from_numpy(pairs), torch.from_numpy(_splits([len(p) for _, p in per_graph]))


def _check(out, expect, what):
    pairs, triples, _ = out
    e_triples, e_pairs, e_splits = expect
    assert torch.equal(triples.row_splits.cpu(), e_splits), what + ": angle_splits"
    assert torch.equal(pairs.row_splits.cpu(), e_splits), what + ": angle_splits of the pairs"
    assert torch.equal(triples.values.cpu(), e_triples), what + ": triples"
    assert torch.equal(pairs.values.cpu(), e_pairs), what + ": pairs"


# ------------------------------------------------------------------------------------------- 1. hand cases, one batch
EMPTY = (np.zeros((0, 3), np.int64), np.zeros((0, 2), np.int64))


def test_hand_cases_as_one_batch(golden_dir):
    cases = load_cases(golden_dir)
    no_edges = np.zeros((0, 2), np.int64)
    # graphs: case 0, case 1, a graph with 3 nodes and no edge, cases 2-4, a graph without nodes
    order = [0, 1, None, 2, 3, 4, None]
    edge_lists = [no_edges if c is None else cases["edges_%d" % c] for c in order]
    node_counts = [int(cases["nodes_%d" % c]) if c is not None else (3 if pos == 2 else 0) for pos, c in enumerate(order)]
    idx, xyz = _batch_of(edge_lists, node_counts)
    for pairing in PAIRINGS:
        for multi in (0, 1):
            for reverse in (0, 1):
                key = "_%s_%d_%d" % (pairing, multi, reverse)
                expect = _expect([EMPTY if c is None else (cases["triples_%d%s" % (c, key)], cases["pairs_%d%s" % (c, key)])
                                  for c in order])
                out = SetAngle(edge_pairing=pairing, allow_multi_edges=bool(multi), allow_reverse_edges=bool(reverse))(
                    idx, xyz)
                _check(out, expect, "hand cases" + key)
                assert out[2].values.shape == (expect[0].shape[0], 1)


def test_batches_without_any_angle(golden_dir):
    cases = load_cases(golden_dir)
    single = cases["edges_3"]                       # one edge: no partner under any rule
    for edge_lists, node_counts in (([single, np.zeros((0, 2), np.int64), single], [2, 4, 2]),
                                    ([np.zeros((0, 2), np.int64)] * 2, [3, 0])):
        idx, xyz = _batch_of(edge_lists, node_counts)
        pairs, triples, theta = SetAngle(edge_pairing="kj")(idx, xyz)
        assert tuple(triples.values.shape) == (0, 3) and tuple(pairs.values.shape) == (0, 2)
        assert tuple(theta.values.shape) == (0, 1) and triples.values.dtype == torch.int64
        assert torch.equal(triples.row_splits.cpu(), torch.zeros(len(node_counts) + 1, dtype=torch.int64))
        assert triples.index_plan(xyz).M == 0 and pairs.index_plan(idx).M == 0


# ------------------------------------------------------------------------------------------- 2. star graphs
LEAVES = (1, 2, 31, 32, 33, 63, 64, 65, 129)


def _star(leaves, sort_receivers):
    """Star with centre 0: both directions of every spoke, interleaved (both columns unsorted) or receiver-sorted."""
    edges = np.array([e for leaf in range(1, leaves + 1) for e in ((0, leaf), (leaf, 0))], dtype=np.int64)
    if sort_receivers:
        edges = edges[np.lexsort((edges[:, 1], edges[:, 0]))]
    return edges


@functools.lru_cache(maxsize=None)
def _star_reference(pairing, sort_receivers):
    return _expect([angle_rule(_star(n, sort_receivers), pairing) for n in LEAVES])


@pytest.mark.parametrize("sort_receivers", [False, True])
@pytest.mark.parametrize("pairing", PAIRINGS)
def test_star_graphs_cross_every_group_boundary(pairing, sort_receivers):
    idx, xyz = _batch_of([_star(n, sort_receivers) for n in LEAVES], [n + 1 for n in LEAVES])
    sa = SetAngle(edge_pairing=pairing)
    first = sa(idx, xyz)
    _check(first, _star_reference(pairing, sort_receivers), "stars " + pairing)
    again = sa(idx, xyz)
    for a, b in zip(first, again):
        assert torch.equal(a.values, b.values) and torch.equal(a.row_splits, b.row_splits)


# ------------------------------------------------------------------------------------------- 3. molecular batches
@functools.lru_cache(maxsize=None)
def _hdnnp():
    return synth.hdnnp_batch(num_graphs=3, seed=21)


@functools.lru_cache(maxsize=None)
def _dimenet():
    return synth.dimenet_batch(num_graphs=3, seed=22)


def _shuffled(b, seed=1):
    """The batch's edge list with the rows of every molecule shuffled, per graph."""
    rng = np.random.default_rng(seed)
    es = b["edge_splits"]
    return [b["edge_indices"][es[g]:es[g + 1]][rng.permutation(int(es[g + 1] - es[g]))] for g in range(len(es) - 1)]


@pytest.mark.parametrize("which", ["hdnnp", "dimenet"])
def test_molecular_batches_sorted_and_shuffled(which):
    b, pairing, col = (_hdnnp(), "kj", 1) if which == "hdnnp" else (_dimenet(), "jk", 0)
    xyz = _rag(b["node_coordinates"], b["node_splits"])
    idx = _rag(b["edge_indices"], b["edge_splits"])
    assert idx.index_plan(xyz).is_sorted(0)
    out = SetAngle(edge_pairing=pairing)(idx, xyz)
    got = out[col]                                   # (pairs, triples, angles): the batch holds triples / pairs
    assert torch.equal(got.values.cpu(), torch.from_numpy(b["angle_indices"])), which
    assert torch.equal(got.row_splits.cpu(), torch.from_numpy(b["angle_splits"])), which
    rows = _shuffled(b)
    idx_s = _rag(np.concatenate(rows, axis=0), b["edge_splits"])
    assert not idx_s.index_plan(xyz).is_sorted(0) and not idx_s.index_plan(xyz).is_sorted(1)
    _check(SetAngle(edge_pairing=pairing)(idx_s, xyz), _expect([angle_rule(r, pairing) for r in rows]),
           which + " shuffled")


# ------------------------------------------------------------------------------------------- 4. attached plans
def _check_plan(idx, nodes, launches_before):
    plan = idx.index_plan(nodes)
    assert _ffi.launch_count() == launches_before, "index_plan launched a kernel: the attached plan was not used"
    assert plan is idx.index_plan(nodes) and any(plan is p for p in idx._plans.values())
    fresh = IndexPlan(RaggedTensor(idx.values, idx.row_splits), nodes)
    assert (plan.M, plan.K, plan.N, plan.G) == (fresh.M, fresh.K, fresh.N, fresh.G)
    assert torch.equal(plan.cols[:, :plan.M], fresh.cols[:, :fresh.M])
    assert not (plan.flags_host() & _ffi.MP_FLAG_OOB)
    if not plan.is_sorted(0):
        assert not fresh.is_sorted(0)               # an unsorted claim is only made where it is true here
    assert torch.equal(plan.csr(0)[0], fresh.csr(0)[0])
    for col in range(plan.K):                       # every column's CSR serves the same buckets
        ptr, perm, _ = plan.csr(col)
        fptr, fperm, _ = fresh.csr(col)
        assert torch.equal(ptr, fptr)
        if perm is not None and fperm is not None:
            assert torch.equal(perm, fperm)
    return plan


@pytest.mark.parametrize("shuffled", [False, True])
def test_attached_plans_equal_fresh_ones(shuffled):
    b = _hdnnp()
    xyz = _rag(b["node_coordinates"], b["node_splits"])
    edges = np.concatenate(_shuffled(b), axis=0) if shuffled else b["edge_indices"]
    idx = _rag(edges, b["edge_splits"])
    pairs, triples, _ = SetAngle(edge_pairing="kj")(idx, xyz)
    before = _ffi.launch_count()
    tplan = _check_plan(triples, xyz, before)
    assert tplan.is_sorted(0) == (not shuffled)
    pplan = _check_plan(pairs, idx, _ffi.launch_count())
    assert pplan.is_sorted(0)


def test_hdnnp2nd_forward_on_device_built_triples():
    from gcnn_keras_amd.literature import HDNNP2nd
    b = _hdnnp()
    model = HDNNP2nd.make_model_behler(**synth.hdnnp_model_kwargs())
    model.set_weights(list(synth.hdnnp_params(seed=10).values()))
    z, xyz = _rag(b["node_number"], b["node_splits"]), _rag(b["node_coordinates"], b["node_splits"])
    idx = _rag(b["edge_indices"], b["edge_splits"])
    host = model([z, xyz, idx, _rag(b["angle_indices"], b["angle_splits"])]).clone()
    _, triples, _ = SetAngle(edge_pairing="kj", compute_angles=False)(idx, xyz)
    device = model([z, xyz, idx, triples])
    assert torch.equal(device, host)


def test_dimenet_forward_on_device_built_pairs():
    from gcnn_keras_amd.literature import DimeNetPP
    b = _dimenet()
    model = DimeNetPP.make_model(**synth.DIMENET_MD17)
    model.set_weights(list(synth.dimenet_params(model, seed=13).values()))
    z, xyz = _rag(b["node_number"], b["node_splits"]), _rag(b["node_coordinates"], b["node_splits"])
    idx = _rag(b["edge_indices"], b["edge_splits"])
    host = model([z, xyz, idx, _rag(b["angle_indices"], b["angle_splits"])]).clone()
    pairs, _, _ = SetAngle(edge_pairing="jk", compute_angles=False)(idx, xyz)
    device = model([z, xyz, idx, pairs])
    assert torch.equal(device, host)


# ------------------------------------------------------------------------------------------- 5. angle values
def _get_angle(coord, indices):
    """The arithmetic of the reference's ``get_angle`` (kgcnn/graph/adj.py:405-414) in the dtype of ``coord``."""
    v1 = coord[indices[:, 0]] - coord[indices[:, 1]]
    v2 = coord[indices[:, 1]] - coord[indices[:, 2]]
    x = np.sum(v1 * v2, axis=-1)
    y = np.linalg.norm(np.cross(v1, v2), axis=-1)
    return np.expand_dims(np.arctan2(y, x), axis=-1)


def test_angle_values_and_compute_angles_off():
    b = _hdnnp()
    xyz = _rag(b["node_coordinates"], b["node_splits"])
    idx = _rag(b["edge_indices"], b["edge_splits"])
    _, triples, theta = SetAngle(edge_pairing="kj")(idx, xyz)
    shift = np.repeat(b["node_splits"][:-1], np.diff(b["angle_splits"]))
    ijk = b["angle_indices"] + shift[:, None]
    ref32 = _get_angle(b["node_coordinates"].astype(np.float32), ijk)
    ref64 = _get_angle(b["node_coordinates"].astype(np.float64), ijk)
    assert ref32.dtype == np.float32 and theta.values.dtype == torch.float32
    assert torch.equal(theta.row_splits, triples.row_splits)
    assert_rows_close(theta.values.cpu().numpy(), ref32, ref64, what="SetAngle angle_attributes")
    off = SetAngle(edge_pairing="kj", compute_angles=False)
    assert off(idx, xyz)[2] is None
    made = off({"range_indices": idx, "node_coordinates": xyz})
    assert sorted(made) == ["angle_indices", "angle_indices_nodes"]


# ------------------------------------------------------------------------------------------- 6. MD driver
MD_ITEMS = [{"name": "node_number", "ragged": True, "dtype": "int64"},
            {"name": "node_coordinates", "ragged": True, "dtype": "float32"},
            {"name": "range_indices", "ragged": True, "dtype": "int64"},
            {"name": "angle_indices_nodes", "ragged": True, "dtype": "int64"}]


def test_md_driver_runs_hdnnp2nd_from_coordinates_alone():
    from gcnn_keras_amd.data.base import MemoryGraphList
    from gcnn_keras_amd.literature import HDNNP2nd
    from gcnn_keras_amd.model.force import EnergyForceModel
    from gcnn_keras_amd.moldyn import MolDynamicsModelPredictor
    b = synth.hdnnp_batch(num_graphs=2, seed=23)
    energy = HDNNP2nd.make_model_behler(**synth.hdnnp_model_kwargs())
    energy.set_weights(list(synth.hdnnp_params(seed=10).values()))
    model = EnergyForceModel(model_energy=energy, coordinate_input=1, energy_output=0, output_as_dict=True,
                             output_to_tensor=False, output_squeeze_states=True)
    ns, es, ts = b["node_splits"], b["edge_splits"], b["angle_splits"]
    graphs = [{"node_number": b["node_number"][ns[i]:ns[i + 1]], "node_coordinates": b["node_coordinates"][ns[i]:ns[i + 1]],
               "range_indices": b["edge_indices"][es[i]:es[i + 1]],
               "angle_indices_nodes": b["angle_indices"][ts[i]:ts[i + 1]]} for i in range(2)]
    bare = [{k: g[k] for k in ("node_number", "node_coordinates")} for g in graphs]
    radius = synth.HDNNP_FORK["cutoff_rad"] + synth.BOHR_PER_ANGSTROM
    outputs = {"energy": "energy", "forces": "force"}
    with_host_lists = MolDynamicsModelPredictor(model=model, model_inputs=MD_ITEMS, model_outputs=outputs)
    on_device = MolDynamicsModelPredictor(
        model=model, model_inputs=MD_ITEMS, model_outputs=outputs,
        tensor_preprocessors=[SetRange(max_distance=radius, max_neighbours=None), SetAngle(edge_pairing="kj")])
    ref = with_host_lists(graphs)
    got = on_device(bare)
    e_ref = np.stack([np.asarray(o["energy"]).reshape(-1) for o in ref])
    f_ref = np.concatenate([np.asarray(o["forces"]) for o in ref], axis=0)
    e_got = np.stack([np.asarray(o["energy"]).reshape(-1) for o in got])
    f_got = np.concatenate([np.asarray(o["forces"]) for o in got], axis=0)
    assert_rows_close(e_got, e_ref, e_ref, what="MD driver with on-device SetRange + SetAngle, energy")
    assert_forces_close(f_got, f_ref, f_ref, ns, what="MD driver with on-device SetRange + SetAngle, forces")
    built = on_device._tensor_input(MemoryGraphList(bare))
    assert torch.equal(built[2].values.cpu(), torch.from_numpy(b["edge_indices"]))
    assert torch.equal(built[2].row_splits.cpu(), torch.from_numpy(es))
    assert torch.equal(built[3].values.cpu(), torch.from_numpy(b["angle_indices"]))
    assert torch.equal(built[3].row_splits.cpu(), torch.from_numpy(ts))
