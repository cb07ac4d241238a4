"""tests/topologies.py on the CPU: the generators deliver the shapes they claim, and on every case the GPU tests of
tests/test_gpu_shape_edges.py run, the float32 torch restatement is itself inside the cap that test applies (the engine
may be twice as far from the float32 restatement as that one is from float64, so the restatement's own distance has to
stay below half the cap; a case that does not meet this gets another seed or value range, never another cap)."""
import numpy as np
import pytest
import torch

import egnn_reference as eref
import topologies as T
from parity import BAR_CAP, assert_forces_close, rowwise_rel

ENC_REV_CAP = 1e-2      # tests/test_gpu_egnn.py: x_bar rows of the edge step


def _half_cap(r32, r64, cap, what):
    for name, a, c in zip(("forward", "reverse 1", "reverse 2"), r32, r64):
        if a.size == 0:
            continue
        e = rowwise_rel(a, c)
        limit = (ENC_REV_CAP if cap == "egnn" and name == "reverse 2" else BAR_CAP) / 2
        print("[restatement] %s %s: float32 is %.2e from float64 (half cap %.1e)" % (what, name, e, limit))
        assert e < limit, "%s %s: float32 restatement %.3g from float64, half cap %.3g" % (what, name, e, limit)


# ------------------------------------------------------------------------------------------------------- generators
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("extras", [False, True])
def test_hub_edges_degrees_ranges_and_boundaries(order, extras):
    n = 200
    e = T.hub_edges(n, T.STANDARD_DEGREES, seed=3, self_loops=extras, duplicates=extras, order=order)
    assert e.dtype == np.int64 and e.shape == (sum(T.STANDARD_DEGREES), 2)
    assert e.min() >= 0 and e.max() < n
    deg = T.in_degrees(e, n)
    assert sorted(deg[deg > 0]) == sorted(T.STANDARD_DEGREES) and np.sum(deg == 0) == n - len(T.STANDARD_DEGREES)
    assert {1, 7, 31, 32, 33, 64, 65, 100} <= set(T.STANDARD_DEGREES) and max(T.STANDARD_DEGREES) >= 1000
    assert deg[0] == 0 and deg[-1] == 0                             # isolated first and last node
    assert np.all(np.diff(e[:, 0]) >= 0) == (order == "sorted")
    loops = int(np.sum(e[:, 0] == e[:, 1]))
    assert loops == (sum(d >= 2 for d in T.STANDARD_DEGREES) if extras else 0)
    if extras:
        for r in np.nonzero(deg >= 3)[0]:
            s = e[e[:, 0] == r, 1]
            assert len(np.unique(s)) < len(s)
    place = T.tile_placement(e, n)
    assert place["starts_on_boundary"] >= 2 and place["ends_on_boundary"] >= 2     # beyond the receiver at offset 0
    assert place["max_whole_tiles"] >= 3
    # deterministic
    assert np.array_equal(e, T.hub_edges(n, T.STANDARD_DEGREES, seed=3, self_loops=extras, duplicates=extras, order=order))


def test_tile_exact_sizes():
    assert set(T.TILE_EXACT_SIZES) == {0, 1, 31, 32, 33, 64}
    for total in T.TILE_EXACT_SIZES:
        n, e = T.tile_exact(total, seed=5)
        assert n == 5 and e.shape == (total, 2) and e.dtype == np.int64
        if total:
            assert e.min() >= 0 and e.max() < n and np.all(np.diff(e[:, 0]) >= 0) and np.all(e[:, 0] != e[:, 1])


def test_degree_edges_put_the_degrees_on_consecutive_nodes():
    degrees = (0, 1, 7, 16, 17, 0, 40, 3)
    for n, first in ((12, 0), (12, 4), (50, 21)):
        e = T.degree_edges(n, degrees, seed=4, first=first)
        assert e.shape == (sum(degrees), 2) and e.dtype == np.int64 and np.all(np.diff(e[:, 0]) >= 0)
        assert e.min() >= 0 and e.max() < n and np.all(e[:, 0] != e[:, 1])
        deg = T.in_degrees(e, n)
        assert tuple(deg[first:first + len(degrees)]) == degrees and deg.sum() == sum(degrees)
        for k, d in enumerate(degrees):                      # senders repeat only where the degree exceeds n - 1
            s = e[e[:, 0] == first + k, 1]
            assert (len(np.unique(s)) == d) == (d <= n - 1)
    assert T.degree_edges(5, (), seed=0).shape == (0, 2)


def test_two_neighbour_edges_have_degree_two_on_both_columns():
    for n in (3, 5, 47, 63):
        e = T.two_neighbour_edges(n)
        assert e.shape == (2 * n, 2) and e.dtype == np.int64 and np.all(np.diff(e[:, 0]) >= 0)
        assert np.all(e[:, 0] != e[:, 1]) and len(np.unique(e, axis=0)) == 2 * n
        assert np.all(T.in_degrees(e, n, 0) == 2) and np.all(T.in_degrees(e, n, 1) == 2)


def test_swap_columns_moves_the_hubs_to_the_sender_side():
    e = T.hub_edges(260, T.STANDARD_DEGREES, seed=3)
    s = T.swap_columns(e)
    assert s.shape == e.shape and s.dtype == np.int64 and s.flags["C_CONTIGUOUS"]
    assert np.array_equal(s[:, 0], e[:, 1]) and np.array_equal(s[:, 1], e[:, 0])
    assert np.all(np.diff(s[:, 1]) >= 0) and np.any(np.diff(s[:, 0]) < 0)
    assert np.array_equal(T.in_degrees(s, 260, column=1), T.in_degrees(e, 260, column=0))


def test_ring_edges_leave_the_other_nodes_isolated():
    n, step = 8209, 3
    e = T.ring_edges(n, step)
    ring = np.arange(0, n, step)
    assert e.shape == (len(ring), 2) and e.dtype == np.int64 and np.all(np.diff(e[:, 0]) > 0)
    assert np.all(e[:, 0] != e[:, 1]) and tuple(e[-1]) == (ring[-1], 0)
    for column in (0, 1):
        deg = T.in_degrees(e, n, column=column)
        assert np.all(deg[ring] == 1) and deg.sum() == len(ring)          # everything off the ring is isolated


@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_hub_triplets_counts(order):
    a = T.hub_triplets(300, T.STANDARD_TRIPLET_COUNTS, seed=11, order=order)
    assert a.shape == (sum(T.STANDARD_TRIPLET_COUNTS), 2) and a.min() >= 0 and a.max() < 300
    assert np.all(a[:, 0] != a[:, 1])
    cnt = T.in_degrees(a, 300)
    assert sorted(cnt[cnt > 0]) == sorted(c for c in T.STANDARD_TRIPLET_COUNTS if c)
    assert {0, 1, 7, 8, 9, 64, 65, 257, 1000} <= set(T.STANDARD_TRIPLET_COUNTS)
    assert {c % 8 for c in T.STANDARD_TRIPLET_COUNTS if c} >= {0, 1, 7}


def test_batches_have_empty_graphs_first_middle_last_and_local_indices():
    for b in (T.egnn_case("hub", seed=3), T.egnn_case("small_hub", seed=6), T.triplet_case(42, seed=11)):
        rs, es = b["row_splits"], b["index_splits"]
        sizes = np.diff(rs)
        assert sizes[0] == 0 and sizes[-1] == 0 and np.any(sizes[1:-1] == 0) and np.sum(sizes > 0) >= 2
        for g in range(len(sizes)):
            rows = b["indices"][es[g]:es[g + 1]]
            assert len(rows) == 0 or (rows.min() >= 0 and rows.max() < sizes[g])
            assert np.array_equal(b["flat"][es[g]:es[g + 1]], rows + rs[g])
    hub = T.egnn_case("hub", seed=3)
    place = T.tile_placement(hub["flat"], hub["rows"])
    assert place["max_whole_tiles"] >= 3 and place["starts_on_boundary"] >= 2 and place["ends_on_boundary"] >= 2
    small = T.egnn_case("small_hub", seed=6)
    assert T.tile_placement(small["flat"], small["rows"])["max_tiles_touched"] >= 4


def test_acsf_case_shapes():
    cases = T.acsf_cases()
    b = cases["many-g2-64-65"][1]
    deg = T.in_degrees(b["ij"], len(b["node_number"]))
    assert deg[0] == 64 and deg[1] == 65 and np.all(deg[2:] == 0)
    assert np.all(T.in_degrees(cases["many-g2-150"][1]["ij"], 150) == 149)
    assert np.all(T.in_degrees(cases["many-g4-40"][1]["ijk"], 40) == 39 * 38)
    for name in ("wide-g2-plain", "wide-g4-target"):
        table = cases[name][2]
        rc = table[..., -1].reshape(-1, table.shape[-2])
        assert table.shape[-2] > 64 and np.all([len(np.unique(row)) == len(row) for row in rc])   # a cutoff per function
        sizes = np.diff(cases[name][1]["node_splits"])
        assert sizes[0] == 0 and sizes[-1] == 0 and np.any(sizes[1:-1] == 0)
    # the relation numbering of the restatement is the layers' own
    from gcnn_keras_amd.layers.conv.acsf_conv import ACSFG2, ACSFG4
    import hdnnp_reference as href
    for elements in (T.ELEMENTS, (1, 6, 7, 8)):
        rmap, pmap, npair = T.pair_maps(elements)
        g4 = ACSFG4(eta_zeta_lambda_rc=T.g4_table(npair, 2, 0), element_mapping=list(elements))
        g2 = ACSFG2(eta_rs_rc=T.g2_table(len(elements), 2, 0), element_mapping=list(elements))
        assert href.tables(g4)[1:] == (rmap, pmap) and href.tables(g2)[1] == rmap
    t = cases["bound-g2-4x512"][2]
    assert t.shape[0] * t.shape[1] == 2048
    t = cases["global-g2-4x171"][2]
    assert t.size > 2048 and t.shape[0] * t.shape[1] <= 2048


def test_large_graph_is_beyond_the_tile_kernels():
    b = T.large_graph_batch()
    n = int(b["node_splits"][-1])
    deg = T.in_degrees(b["edge_indices"], n)
    assert n > 4096 and len(b["node_splits"]) == 2 and 8 <= deg.min() and deg.max() <= 12
    assert np.all(np.diff(b["edge_indices"][:, 0]) >= 0) and np.all(b["edge_indices"][:, 0] != b["edge_indices"][:, 1])


# ------------------------------------------------------------------------------------------------------- restatements
@pytest.mark.parametrize("name", sorted(T.egnn_cases()))
def test_egnn_cases_float32_restatement_inside_half_the_cap(name):
    case = T.egnn_case(**T.egnn_cases()[name])
    r32, r64 = T.egnn_restate(case, torch.float32), T.egnn_restate(case, torch.float64)
    _half_cap(r32, r64, "egnn", "EGNN %s" % name)
    deg = T.in_degrees(case["flat"], case["rows"])
    assert np.all(r64[0][deg == 0] == 0)


def test_egnn_restatement_on_the_default_encoding_is_the_reference_one():
    case = T.egnn_case("small_hub", seed=6)
    w = case["weights"]
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    _, m_i = eref.edge_step(t(case["h"]), t(case["x"]), torch.from_numpy(case["flat"]),
                            [(t(w["w1"]), t(w["b1"]), "swish"), (t(w["w2"]), t(w["b2"]), "swish")],
                            [(t(w["wa"]), t(w["ba"]), "sigmoid")], torch.float64, expand=True)
    assert np.array_equal(m_i.numpy(), T.egnn_restate(case, torch.float64)[0])


def test_egnn_model_case_forces_of_the_float32_restatement():
    """The model-level case of the GPU test: 70-atom molecule (in-degree 69), cutoff as tests/test_gpu_egnn.py explains."""
    from gcnn_keras_amd import synth
    from gcnn_keras_amd.literature import EGNN
    b = synth.egnn_batch(**T.EGNN_MODEL_BATCH)
    deg = np.bincount(eref.flat_edges(b)[:, 0], minlength=len(b["node_coordinates"]))
    assert deg.max() == 69
    m = EGNN.make_model(**synth.EGNN_MD17)
    p = list(synth.egnn_params(m, seed=14).values())
    e64, f64 = eref.energy_forces(p, b, m.config, dtype=torch.float64)
    e32, f32 = eref.energy_forces(p, b, m.config, dtype=torch.float32)
    assert rowwise_rel(e32.numpy(), e64.numpy()) < BAR_CAP / 2
    ns = b["node_splits"]
    for g in range(len(ns) - 1):
        if ns[g + 1] > ns[g] and float(f64[ns[g]:ns[g + 1]].abs().max()) > 0:
            e = float((f32 - f64)[ns[g]:ns[g + 1]].abs().max() / f64[ns[g]:ns[g + 1]].abs().max())
            print("[restatement] EGNN model case molecule %d: float32 forces %.2e of the scale from float64" % (g, e))
            assert e < BAR_CAP / 2
    assert_forces_close(f32.numpy(), f32.numpy(), f64.numpy(), ns, what="EGNN model case, float32 restatement")


@pytest.mark.parametrize("nsbf", T.TRIPLET_WIDTHS + (65,))
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_triplet_cases_float32_restatement_inside_half_the_cap(nsbf, order):
    case = T.triplet_case(nsbf, order, seed=11)
    r32, r64 = T.triplet_restate(case, torch.float32), T.triplet_restate(case, torch.float64)
    _half_cap(r32, r64, None, "triplet step nsbf=%d %s" % (nsbf, order))
    assert np.all(r64[0][T.in_degrees(case["flat"], case["rows"]) == 0] == 0)


@pytest.mark.parametrize("shuffled", [False, True])
def test_many_triplets_batch_and_its_angle_restatement(shuffled):
    import dimenet_reference as dref
    b = T.many_triplets_batch(shuffled)
    ei, ai = (torch.from_numpy(a) for a in dref.flat_indices(b))
    count = np.bincount(ai[:, 0].numpy(), minlength=len(ei))
    assert count.max() == 70 and np.all(count[:72 * 71] == 70)           # more than one 64-lane round on every edge
    assert bool(np.all(np.diff(ai[:, 0].numpy()) >= 0)) == (not shuffled)
    g = np.random.default_rng(3).normal(size=(len(ai),)).astype(np.float32)
    outs = {}
    for dt in (torch.float32, torch.float64):
        x = torch.tensor(b["node_coordinates"], dtype=dt)
        v = (x[ei[:, 0]] - x[ei[:, 1]]).detach().requires_grad_(True)
        t = dref.vector_angle(v[ai[:, 0]], v[ai[:, 1]])
        (gv,) = torch.autograd.grad(t, [v], torch.tensor(g, dtype=dt))
        outs[dt] = (t.detach().numpy()[:, None], gv.numpy())
    # the spherical-basis rows are held to the float32 restatement's own distance (SBF_CAP = 1 in tests/test_gpu_dimenet.py)
    _half_cap(outs[torch.float32], outs[torch.float64], None, "72 atoms edge angle%s" % (" shuffled" if shuffled else ""))


@pytest.mark.parametrize("name", sorted(T.acsf_cases()))
def test_acsf_cases_float32_restatement_inside_half_the_cap(name):
    kind, b, table, mult, with_jvp = T.acsf_cases()[name]
    g, h = T.acsf_upstream(name, b, table.shape[-3] * table.shape[-2])
    r32, r64 = (T.acsf_restate(kind, b, table, dt, T.acsf_elements(name), mult, h if with_jvp else None, g)
                for dt in (torch.float32, torch.float64))
    order = (0, 1, 2) if with_jvp else (0, 1)
    _half_cap([r32[k] for k in order], [r64[k] for k in order], None, "ACSF %s" % name)
    assert float(np.max(np.abs(r64[0]))) > 0


def test_large_graph_force_oracle_float32_inside_half_the_cap():
    from gcnn_keras_amd import synth
    from oracle import torch_force_oracle as tfo
    b = T.large_graph_batch()
    p = synth.painn_params(seed=8, random_bias=True)
    (e32, f32), (e64, f64) = (tfo.painn_energy_force(p, b, dt, equiv_method="eps", cutoff=None)
                              for dt in (torch.float32, torch.float64))
    f32, f64 = np.asarray(f32), np.asarray(f64)
    assert float(np.max(np.abs(f32 - f64)) / np.max(np.abs(f64))) < BAR_CAP / 2
    assert rowwise_rel(np.asarray(e32).reshape(-1, 1), np.asarray(e64).reshape(-1, 1)) < BAR_CAP / 2
