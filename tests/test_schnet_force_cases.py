"""tests/schnet_force_cases.py on the CPU: every generator delivers the boundary it claims (basis sizes against the FP32
build of the distance gradient, edge counts against tile, workgroup and grid, degrees against the 64 lanes of the force
kernel, node and graph counts against the persistent grids, graph sizes against the readout's rounds), and on every case
tests/test_gpu_schnet_force_edges.py compares, the float32 restatement is at most half the bar that test applies, in the
metric it applies (the engine may be as far from the float32 restatement as that one is from float64; a case that does
not meet this is changed, the bar stays).  Each distance is printed; the table in the GPU file's docstring is a copy."""
import numpy as np
import pytest
import torch

import schnet_force_cases as C
import topologies as T
from gcnn_keras_amd import synth
from oracle import torch_force_oracle as tfo
from parity import BAR_CAP, RTOL, assert_forces_close, rowwise_rel


def _half(what, r32, r64, bar):
    e = C.max_rel(r32, r64)
    print("[restatement] %s: float32 is %.2e of the largest magnitude from float64 (half bar %.1e)" % (what, e, bar / 2))
    assert e <= bar / 2, "%s: float32 restatement %.3g from float64, half bar %.3g" % (what, e, bar / 2)
    return e


def _half_rows(what, r32, r64):
    """assert_rows_close with the float64 twin: the bar is max(RTOL, min(2 x this distance, BAR_CAP)); the restatement is
    within half of it exactly when it is within BAR_CAP / 2.  Held to RTOL / 2 here: the bar then stays at RTOL."""
    e = rowwise_rel(r32, r64)
    print("[restatement] %s: float32 rows are %.2e from float64 (half bar %.1e)" % (what, e, RTOL / 2))
    assert e <= RTOL / 2 <= BAR_CAP / 2, "%s: float32 restatement %.3g from float64" % (what, e)
    return e


# ------------------------------------------------------------------------------------- A. distance gradient
def test_thresholds_of_the_distance_gradient_kernel():
    assert [b for b in range(1, C.MAX_BINS + 1) if C.fp32_basis_build(b)] == [32]
    assert ((32 + 2) >> 1) > 16 and ((31 + 2) >> 1) == 16 and ((1 + 2) >> 1) == 1 and ((2 + 2) >> 1) == 2
    assert C.EDGE_TILE == T.TILE == 32 and C.EDGE_WORKGROUP == 128 and C.EDGE_TRIP == 32768
    names = C.dist_grad_cases()
    assert {names["bins%d" % b]["bins"] for b in (1, 2, 30, 31, 32)} == {1, 2, 30, 31, 32}
    assert names["trip-bins32"]["bins"] == 32 and names["bins32-nobias"]["bins"] == 32


@pytest.mark.parametrize("name", sorted(C.dist_grad_cases()))
def test_distance_gradient_cases(name):
    kw = C.dist_grad_cases()[name]
    c = C.dist_grad_case(**kw)
    n, m = c["N"], c["M"]
    assert c["x"].shape == c["g_out"].shape == (n, C.F) and c["w1"].shape == (c["bins"], C.F) and c["dist"].shape == (m,)
    assert all(np.float32(c[k]) == c[k] for k in ("distance", "sigma", "offset"))
    assert (c["b1"] is None) == name.endswith("nobias")
    tiles, groups = -(-m // C.EDGE_TILE), -(-m // C.EDGE_WORKGROUP)
    ordinary = np.setdiff1d(np.arange(m), c["marked"])
    if name.startswith("bins") or kw["graph"] == "small":
        assert n == 40 and m == 1300 and groups == 11
    if name.startswith("exact"):
        assert n == 5 and m == int(name[5:]) and m in (1, 31, 32, 33, 127, 128, 129)
        assert tiles == {1: 1, 31: 1, 32: 1, 33: 2, 127: 4, 128: 4, 129: 5}[m]
        assert (tiles < 4) == (m <= 96)                                   # fewer tiles than the workgroup has waves
    if name.startswith("trip"):
        assert n == 40 and m == C.EDGE_TRIP + 33 and m > 32768 and groups > C.EDGE_GRID
        assert tiles - C.EDGE_GRID * 4 == 2 and m % C.EDGE_TILE == 1      # the second trip: one whole tile, one of one edge
        assert C.fp32_basis_build(c["bins"]) == (name == "trip-bins32")
    if name == "nine-workgroups":
        assert groups == 9 and groups % 8 != 0 and groups < C.EDGE_GRID
    if name.startswith("hub"):
        e = np.stack([c["recv"], c["send"]], axis=-1).astype(np.int64)
        deg = T.in_degrees(e, n)
        assert n == 260 and sorted(deg[deg > 0]) == sorted(T.STANDARD_DEGREES) and c["distance"] == 8.0
        is_sorted = bool(np.all(np.diff(c["recv"]) >= 0))
        assert is_sorted == (name != "hub-shuffled")
        if is_sorted:
            place = T.tile_placement(e, n)
            assert place["max_whole_tiles"] == 30 and place["starts_on_boundary"] >= 2 and place["ends_on_boundary"] >= 2
        loops = c["recv"] == c["send"]
        assert int(loops.sum()) == (8 if name == "hub-selfdup" else 0)
        assert np.array_equal(c["dist"] == 0, loops)                      # a self loop has d = 0 and a basis slope != 0
        if name == "hub-selfdup":
            assert len(np.unique(e, axis=0)) < m                          # duplicated pairs
    if c["special"] == "zero":
        assert np.all(c["dist"][c["marked"]] == 0) and np.all(c["dist"][ordinary] > 0) and len(c["marked"]) == 8
    if c["special"] == "far":
        assert np.all(c["dist"][c["marked"]] == np.float32(3 * c["distance"])) and c["dist"][ordinary].max() < 10
    if name == "offset":
        assert c["offset"] == 0.75
    if name == "sigma0.1":
        assert c["sigma"] == float(np.float32(0.1))
    pre = C.pre1_of(c)
    if c["special"] == "saturated":
        assert abs(np.abs(pre).max() - C.SATURATED_PRE) < 0.5 and (pre > 50).any() and (pre < -50).any()
    else:
        assert np.abs(pre).max() < 10
    if c["special"] == "oob":
        bad = (c["recv"] < 0) | (c["recv"] >= n) | (c["send"] < 0) | (c["send"] >= n)
        assert np.array_equal(np.nonzero(bad)[0], c["marked"]) and len(c["marked"]) == 5
        assert {int(v) for v in c["recv"][bad]} | {int(v) for v in c["send"][bad]} >= {-1, n}
    else:
        assert c["recv"].min() >= 0 and c["recv"].max() < n and c["send"].min() >= 0 and c["send"].max() < n
    r32, r64 = C.dist_grad_restate(c, np.float32), C.dist_grad_restate(c, np.float64)
    assert r32.dtype == np.float32 and r64.dtype == np.float64 and np.all(np.isfinite(r64))
    # the scale is set by ordinary edges: the marked ones are not the largest entries
    assert np.abs(r64[ordinary]).max() == np.abs(r64).max() or c["special"] in (None, "saturated")
    if c["special"] == "zero":
        assert np.all(r64[c["marked"]] != 0)                              # d = 0 is not a silent edge
    if c["special"] == "far":
        assert np.all(np.abs(r64[c["marked"]]) < 1e-100) and not r32[c["marked"]].any()   # far outside the basis
    _half("g_d %s (N %d, M %d, bins %d)" % (name, n, m, c["bins"]), r32, r64, C.BAR_CHAIN)


def test_distance_gradient_restatement_is_the_derivative_of_the_filter():
    """Central differences of ``sum_e sum_f g_out[recv, f] x[send, f] w_f(d_e)`` in float64 against the restatement."""
    c = C.dist_grad_case(graph="exact33", bins=7, offset=0.25)
    c["dist"] = c["dist"].astype(np.float64)
    v = c["g_out"][c["recv"]].astype(np.float64) * c["x"][c["send"]].astype(np.float64)

    def energy_terms(d):
        cc = dict(c, dist=d)
        gauss, _ = C._basis(cc, np.float64)
        return np.sum(v * (C._ssp(gauss @ c["w1"].astype(np.float64) + c["b1"]) @ c["w2"].astype(np.float64)), axis=1)

    h = 1e-6
    num = (energy_terms(c["dist"] + h) - energy_terms(c["dist"] - h)) / (2 * h)
    want = C.dist_grad_restate(c, np.float64)
    assert np.max(np.abs(num - want)) <= 1e-7 * np.max(np.abs(want))


# ------------------------------------------------------------------------------------- B. forces from dE/dd
@pytest.mark.parametrize("name", sorted(C.force_cases()))
def test_force_cases(name):
    c = C.force_case(**C.force_cases()[name])
    n, m, e = c["N"], c["M"], c["edges"]
    deg0, deg1 = T.in_degrees(e, n, 0), T.in_degrees(e, n, 1)
    sorted0, sorted1 = bool(np.all(np.diff(e[:, 0]) >= 0)), bool(np.all(np.diff(e[:, 1]) >= 0))
    hubs = {64, 65, 100, 1000}
    if name == "receiver-hubs":
        assert sorted0 and not sorted1 and hubs <= set(deg0) and deg0.max() > C.FORCE_LANES     # perm0 None
    if name == "sender-hubs":
        assert sorted1 and not sorted0 and hubs <= set(deg1) and deg1.max() > C.FORCE_LANES     # perm1 None
    if name == "shuffled-hubs":
        assert not sorted0 and not sorted1 and hubs <= set(deg0)
    if name == "hubs-selfdup-plus":
        assert int(np.sum(e[:, 0] == e[:, 1])) == 8 and c["scale"] == 1.0
    else:
        assert c["scale"] == -1.0
    if name == "node-trip":
        assert n == 8192 + 17 and n > C.FORCE_WAVES and sorted0
        isolated = (deg0 == 0) & (deg1 == 0)
        assert isolated.sum() == n - len(e)
        assert not isolated[C.FORCE_WAVES + 1] and isolated[C.FORCE_WAVES + 2]      # the second trip holds both kinds
    if name == "no-edges":
        assert m == 0 and n > 0
    zero = c["dist"] == 0
    loops = e[:, 0] == e[:, 1]
    if m:
        assert len(c["coincident"]) == 2 and np.all(zero[c["coincident"]]) and not np.any(loops[c["coincident"]])
        assert np.all(zero[loops]) and np.all(c["dist"][~zero] > 0.05)
    r32, r64 = C.force_restate(c, np.float32), C.force_restate(c, np.float64)
    assert r32.dtype == np.float32 and r64.shape == (n, 3)
    assert np.all(r64[(deg0 == 0) & (deg1 == 0)] == 0)
    if m == 0:
        assert not r64.any()
        return
    # an edge at d = 0 contributes nothing: dropping those edges changes no bit
    keep = dict(c, **{k: c[k][~zero] for k in ("recv", "send", "dist", "g_d")})
    assert np.array_equal(C.force_restate(keep, np.float64), r64)
    assert np.max(np.abs(r64.sum(0))) <= 1e-9 * np.abs(r64).max()       # actio = reactio
    _half("forces %s (N %d, M %d)" % (name, n, m), r32, r64, C.BAR_FORCE)


# ------------------------------------------------------------------------------------- C. SAVE node chains
def test_node_counts_reach_the_tile_edges_and_the_second_trip():
    assert C.NODE_COUNTS == (1, 15, 16, 17, 8193)
    assert C.NODE_COUNTS[-1] > 512 * 16 and -(-C.NODE_COUNTS[-1] // C.NODE_TILE) == C.NODE_GRID + 1
    assert {n % C.NODE_TILE for n in C.NODE_COUNTS} == {0, 1, 15}


@pytest.mark.parametrize("n,bias,saturated", [(n, True, False) for n in C.NODE_COUNTS] + [(17, False, False),
                                                                                        (8193, False, False),
                                                                                        (37, True, True)])
def test_node_chain_cases(n, bias, saturated):
    c = C.node_case(n, bias=bias, saturated=saturated)
    assert all((c[k] is None) == (not bias) for k in ("b2", "b3", "bl0", "bl1"))
    assert c["agg"].shape == c["n"].shape == (n, C.F) and c["Wl1"].shape == (C.F, C.H)
    r32, r64 = C.node_restate(c, np.float32), C.node_restate(c, np.float64)
    if saturated:
        for k in ("pre2", "prel0"):
            assert abs(np.abs(r64[k]).max() - C.SATURATED_SPAN) < 0.5 and r64[k].max() > 20 and r64[k].min() < -20
        assert np.abs(r64["prel1"]).max() > 10
        for k in ("d2", "dl0", "dl1"):        # saturated sigmoids: the ends of [0, 1] are reached to 1e-10, nothing leaves it
            assert np.all(np.isfinite(r32[k])) and r32[k].min() >= 0 and r32[k].max() <= 1
        assert r64["d2"].min() < 1e-10 and r64["d2"].max() > 1 - 1e-10
    else:
        assert np.abs(r64["pre2"]).max() < 8
    tag = "n=%d%s%s" % (n, "" if bias else " no bias", " saturated" if saturated else "")
    for k in sorted(set(C.MID_OUTPUTS + C.LAST_OUTPUTS)):
        assert r32[k].dtype == np.float32
        _half("node chains %s %s" % (tag, k), r32[k], r64[k], C.BAR_CHAIN)


# ------------------------------------------------------------------------------------- D. readout
def test_readout_sizes_reach_every_round_and_the_second_trip():
    s = C.READOUT_SIZES
    assert s == (0, 1, 7, 8, 9, 23, 24, 25, 33, 100, 0, 16, 0)
    assert s[0] == 0 and s[-1] == 0 and 0 in s[1:-1]
    for edge in (8, 16, 24):                                  # both sides of every prefetch round
        assert any(v <= edge for v in s if v > edge - 8) and any(v > edge for v in s)
    assert {7, 8, 9, 16, 23, 24, 25} <= set(s) and max(s) > C.READOUT_PREFETCH + C.READOUT_ROUND
    t = C.readout_trip_sizes()
    assert len(t) == 4096 + 5 and len(t) > C.READOUT_WAVES and set(t) == {0, 1, 2}
    assert t[C.READOUT_WAVES:].sum() > 0                      # the second trip pools real rows


@pytest.mark.parametrize("sizes", ["edges", "trip"])
@pytest.mark.parametrize("bias", [(True, True), (False, True), (True, False)])
def test_readout_cases(sizes, bias):
    c = C.readout_case(C.READOUT_SIZES if sizes == "edges" else C.readout_trip_sizes(), bias=bias)
    assert c["splits"].dtype == np.int64 and c["splits"][-1] == c["N"] and np.array_equal(np.diff(c["splits"]), c["sizes"])
    assert (c["bo0"] is None) == (not bias[0]) and (c["bo1"] is None) == (not bias[1])
    empty = c["sizes"] == 0
    tag = "%s bo0=%d bo1=%d" % (sizes, bias[0], bias[1])
    o32, g32 = C.readout_restate(c, np.float32)
    o64, g64 = C.readout_restate(c, np.float64)
    b0 = np.zeros(C.H) if c["bo0"] is None else c["bo0"].astype(np.float64)
    b1 = 0.0 if c["bo1"] is None else float(c["bo1"][0])
    want_empty = C._ssp(b0) @ c["Wo1"][:, 0].astype(np.float64) + b1            # out of a graph without rows
    assert np.allclose(o64[empty, 0], want_empty, rtol=1e-14, atol=0)
    assert np.all(g64[empty] == g64[empty][0]) and (np.abs(g64[empty][0]).max() > 0)
    _half_rows("readout MLP head %s out" % tag, o32, o64)
    _half_rows("readout MLP head %s g_pool" % tag, g32, g64)
    l32, none = C.readout_restate(c, np.float32, head="linear")
    l64, _ = C.readout_restate(c, np.float64, head="linear")
    assert none is None and np.all(l64[empty] == 0) and np.all(l64[~empty] != 0)
    _half_rows("readout linear head %s out" % tag, l32, l64)


# ------------------------------------------------------------------------------------- E. composed batch
@pytest.mark.parametrize("bins", [32, 25])
@pytest.mark.parametrize("shuffled", [False, True])
def test_model_batch_and_the_float32_reference(bins, shuffled):
    b = C.model_batch(synth.radius_graph, shuffled=shuffled)
    ns, es = b["node_splits"], b["edge_splits"]
    assert list(np.diff(ns)) == [70, 1, 0, 21] and list(np.diff(es))[1:3] == [0, 0]
    e0 = b["edge_indices"][es[0]:es[1]]
    for column in (0, 1):
        deg = T.in_degrees(e0, 70, column)
        assert deg.min() > C.FORCE_LANES and deg.max() == 69                   # two lane rounds on both sides
    assert bool(np.all(np.diff(e0[:, 0]) >= 0)) == (not shuffled)
    sorted_b = C.model_batch(synth.radius_graph)
    assert np.array_equal(b["node_coordinates"], sorted_b["node_coordinates"])
    for g in range(4):                                                         # the same pairs, graph by graph
        a, s = b["edge_indices"][es[g]:es[g + 1]], sorted_b["edge_indices"][es[g]:es[g + 1]]
        assert np.array_equal(a[np.lexsort((a[:, 1], a[:, 0]))], s)
    ga = C.MODEL_GAUSS[bins]
    assert ga["bins"] == bins and ga["distance"] == 8 and C.fp32_basis_build(bins) == (bins == 32)
    if shuffled and bins == 25:
        return                                                                 # (the reference runs once per basis below)
    p = synth.schnet_params(seed=7, bins=bins, random_bias=True)
    (e32, f32), (e64, f64) = (tfo.schnet_energy_force(p, b, dt, depth=3, gauss_args=ga)
                              for dt in (torch.float32, torch.float64))
    tag = "SchNet model bins %d %s" % (bins, "shuffled" if shuffled else "sorted")
    _half_rows(tag + " energy", e32, e64)
    for g in range(len(ns) - 1):
        lo, hi = ns[g], ns[g + 1]
        if hi > lo and np.abs(f64[lo:hi]).max() > 0:
            e = C.max_rel(f32[lo:hi], f64[lo:hi])
            print("[restatement] %s molecule %d: float32 forces %.2e of the scale from float64" % (tag, g, e))
            assert e <= BAR_CAP / 2
    assert np.all(f64[70] == 0)                                                # the lone atom
    assert_forces_close(f32, f32, f64, ns, what=tag + ", float32 reference")
