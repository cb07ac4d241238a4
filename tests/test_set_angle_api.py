"""On-GPU ``SetAngle``: the host surface (constructor, config, ``produces``, errors) and the rule itself - a brute-force
NumPy restatement kept here (``angle_rule``, also the yardstick of tests/test_gpu_set_angle.py) reproduces the
reference's ``get_angle_indices`` output stored in tests/golden/angle_cases.npz bit for bit.  Runs without a GPU."""
import os

import numpy as np
import pytest

from gcnn_keras_amd.graph.preprocessor import SetAngle

PAIRINGS = ("jk", "ik", "kj", "ki")
NUM_CASES = 5


def angle_rule(idx, edge_pairing="kj", allow_multi_edges=False, allow_reverse_edges=False):
    """``(triples (A, 3), pairs (A, 2))`` of one graph's edge list ``idx (M, 2)``, edge by edge: the partners of edge
    ``n = (i, j)`` are the edges ``m != n`` with ``idx[m, pos_fix] == idx[n, pos_ij]``, without copies of ``(i, j)``
    unless multi edges and copies of ``(j, i)`` unless reverse edges are allowed; ordered by ``n``, then ``m``."""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1, 2)
    pos_k = edge_pairing.index("k")
    pos_fix = 1 - pos_k
    pos_ij = 0 if "i" in edge_pairing else 1
    triples, pairs = [], []
    for n, (i, j) in enumerate(idx):
        for m, e in enumerate(idx):
            if m == n or e[pos_fix] != idx[n, pos_ij]:
                continue
            if not allow_multi_edges and e[0] == i and e[1] == j:
                continue
            if not allow_reverse_edges and e[0] == j and e[1] == i:
                continue
            triples.append((i, j, e[pos_k]))
            pairs.append((n, m))
    return np.array(triples, np.int64).reshape(-1, 3), np.array(pairs, np.int64).reshape(-1, 2)


def load_cases(golden_dir):
    return np.load(os.path.join(golden_dir, "angle_cases.npz"), allow_pickle=False)


def test_constructor_and_config_mirror_the_reference():
    cfg = SetAngle().get_config()
    assert cfg == {"name": "set_angle", "node_coordinates": "node_coordinates", "range_indices": "range_indices",
                   "angle_indices": "angle_indices", "angle_indices_nodes": "angle_indices_nodes",
                   "angle_attributes": "angle_attributes", "allow_multi_edges": False, "compute_angles": True,
                   "allow_self_edges": False, "edge_pairing": "kj", "allow_reverse_edges": False, "check_sorted": True}
    sa = SetAngle(range_indices="edge_indices", node_coordinates="xyz", angle_indices="a", angle_indices_nodes="an",
                  angle_attributes="aa", allow_multi_edges=True, allow_reverse_edges=True, edge_pairing="ik",
                  check_sorted=False, compute_angles=False, name="angles")
    cfg = sa.get_config()
    assert cfg["name"] == "angles" and cfg["range_indices"] == "edge_indices" and cfg["node_coordinates"] == "xyz"
    assert cfg["edge_pairing"] == "ik" and cfg["check_sorted"] is False and cfg["compute_angles"] is False
    assert cfg["allow_multi_edges"] is True and cfg["allow_reverse_edges"] is True
    assert SetAngle(**cfg).get_config() == cfg     # round trip, as the reference's preprocessors are rebuilt


def test_produces_lists_the_new_properties():
    assert SetAngle().produces == ("angle_indices", "angle_indices_nodes", "angle_attributes")
    assert SetAngle(compute_angles=False).produces == ("angle_indices", "angle_indices_nodes")
    assert SetAngle(angle_indices="a", angle_indices_nodes="an", angle_attributes="aa").produces == ("a", "an", "aa")


@pytest.mark.parametrize("pairing,pos", [("jk", (1, 0, 1)), ("ik", (1, 0, 0)), ("kj", (0, 1, 1)), ("ki", (0, 1, 0))])
def test_pairing_positions(pairing, pos):
    sa = SetAngle(edge_pairing=pairing)
    assert (sa.pos_k, sa.pos_fix, sa.pos_ij) == pos


def test_errors():
    with pytest.raises(NotImplementedError):
        SetAngle(allow_self_edges=True)
    with pytest.raises(ValueError, match="Edge pairing must have index 'k'."):
        SetAngle(edge_pairing="ij")
    with pytest.raises(ValueError, match="Edge pairing must have at least one fix index 'i' or 'j'."):
        SetAngle(edge_pairing="kl")


def test_rule_restatement_reproduces_the_reference(golden_dir):
    cases = load_cases(golden_dir)
    total = 0
    for c in range(NUM_CASES):
        edges = cases["edges_%d" % c]
        for pairing in PAIRINGS:
            for multi in (0, 1):
                for reverse in (0, 1):
                    key = "%d_%s_%d_%d" % (c, pairing, multi, reverse)
                    triples, pairs = angle_rule(edges, pairing, bool(multi), bool(reverse))
                    assert np.array_equal(triples, cases["triples_" + key]), key
                    assert np.array_equal(pairs, cases["pairs_" + key]), key
                    assert triples.dtype == cases["triples_" + key].dtype == np.int64
                    total += len(pairs)
    assert total > 500       # the fixture is not trivially empty


def test_rule_restatement_equals_the_synth_helpers():
    from gcnn_keras_amd import synth
    edges = synth.radius_graph(np.random.default_rng(3).normal(0.0, 1.5, size=(9, 3)).astype(np.float32),
                               max_distance=3.0, max_neighbours=None)
    assert len(edges) > 10
    assert np.array_equal(angle_rule(edges, "kj")[0], synth.angle_indices(edges, "kj"))
    assert np.array_equal(angle_rule(edges, "ik")[0], synth.angle_indices(edges, "ik"))
    assert np.array_equal(angle_rule(edges, "jk")[1], synth.angle_pairs(edges, "jk"))
