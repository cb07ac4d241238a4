"""tests/painn_cases.py on the CPU: every generator delivers the boundary it claims (degrees against the 16-edge step, its
8-edge half, the 64-edge round and the ``EC`` tails, tile counts against the 2048 workgroups, node counts against the
gather pair's waves and the update pair's tiles, graph counts against ``PREP_LDS_GRAPHS``, LDS need against 160 KB through
the library's host probes), and on every case tests/test_gpu_painn_edges.py compares, the float32 restatement is at most
half the bar that test applies, in the metric it applies (a case that does not meet this is changed, the bar stays).
Each distance is printed; the table in the GPU file's docstring is a copy."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import painn_cases as C
import topologies as T
from gcnn_keras_amd import _ffi, synth
from gcnn_keras_amd.fused_painn import message_tile_table
from oracle import torch_force_oracle as tfo
from parity import BAR_CAP, FORCE_RTOL, RTOL, assert_forces_close, rowwise_rel


def _half(what, r32, r64, bar):
    e = C.max_rel(r32, r64)
    print("[restatement] %s: float32 is %.2e of the largest magnitude from float64 (half bar %.1e)" % (what, e, bar / 2))
    assert e <= bar / 2, "%s: float32 restatement %.3g from float64, half bar %.3g" % (what, e, bar / 2)


def _half_rows(what, r32, r64):
    """assert_rows_close with the float64 twin keeps its bar at RTOL while the float32 restatement is within RTOL / 2."""
    e = rowwise_rel(r32, r64)
    print("[restatement] %s: float32 rows are %.2e from float64 (half bar %.1e)" % (what, e, RTOL / 2))
    assert r32.dtype == np.float32 and r64.dtype == np.float64
    assert e <= RTOL / 2 <= BAR_CAP / 2, "%s: float32 restatement %.3g from float64" % (what, e)


@functools.lru_cache(maxsize=None)
def _case(direction, name):
    return C.message_case(**(C.FORWARD_RUNS if direction == "fwd" else C.REVERSE_RUNS)[name][0])


def _table(c, per, reverse):
    col = c["send"] if reverse else c["recv"]
    ptr, _ = C.csr(col, c["N"])
    return message_tile_table(c["node_splits"], ptr, c["B"], per=per, reverse=reverse)


# ------------------------------------------------------------------------------------- thresholds and LDS formulas
def test_thresholds():
    assert (C.STEP_EDGES, C.HALF_STEP, C.TILE_NODES, C.TILE_GRID, C.GATHER_ROUND) == (16, 8, 62, 2048, 64)
    assert (C.EC_FWD, C.EC_BWD, C.GATHER_WAVES, C.UPDATE_TILE, C.UPDATE_GRID) == (8, 4, 16384, 16, 256)
    assert C.PREP_LDS_GRAPHS == 1023 and C.LDS_LIMIT == 163840 and C.ACT_SWISH == _ffi.activation_code("swish")
    assert [C.kgroups(b) for b in (1, 7, 8, 15, 16, 20, 23, 24, 31)] == [1, 1, 2, 2, 3, 3, 3, 4, 4]
    assert C.UPDATE_COUNTS == (1, 15, 16, 17, 4097) and C.UPDATE_COUNTS[-1] > 256 * 16
    assert -(-C.UPDATE_COUNTS[-1] // C.UPDATE_TILE) == C.UPDATE_GRID + 1            # one tile on the second trip
    assert C.RING_NODES == 8209 and 2 * C.RING_NODES > 4096 * 4


def test_lds_formulas_equal_the_host_probes():
    lds = ctypes.c_size_t(0)
    for rows in (1, 2, 21, 48, 49, 50, 57, 63):
        for edges in (0, 1, 15, 16, 17, 63, 64, 96, 110, 564):
            for basis in (1, 7, 8, 10, 20, 31):
                for env in (0, 1):
                    _ffi.call("mp_painn_message_tiles_lds_bytes", rows, edges, basis, env, ctypes.byref(lds))
                    assert lds.value == C.fwd_tile_lds_bytes(rows, edges, basis, bool(env)), (rows, edges, basis, env)
                    for senders in (1, 2, 3, 24, 62):
                        _ffi.call("mp_painn_message_bwd_tiles_lds_bytes", rows, senders, edges, basis, env, ctypes.byref(lds))
                        assert lds.value == C.bwd_tile_lds_bytes(rows, senders, edges, basis, bool(env))
    # the figures the tile tables turn on: complete graphs, two nodes per tile, 20 basis functions, envelope counted
    assert C.fwd_tile_lds_bytes(49, 2 * 48, 20) == 163584 and C.fwd_tile_lds_bytes(50, 2 * 49, 20) == 165888
    assert C.fwd_tile_lds_bytes(48, 2 * 47, 31) <= C.LDS_LIMIT < C.fwd_tile_lds_bytes(49, 2 * 48, 31)
    assert C.fwd_tile_lds_bytes(50, 2 * 49, 10) <= C.LDS_LIMIT < C.fwd_tile_lds_bytes(51, 2 * 50, 10)
    assert C.bwd_tile_lds_bytes(56, 2, 2 * 55, 20) == 163072 and C.bwd_tile_lds_bytes(57, 2, 2 * 56, 20) > C.LDS_LIMIT
    # a graph's rows alone bound a forward tile to 53 nodes, the reverse one to 80: the 62-node clamp is out of reach forward
    assert C.fwd_tile_lds_bytes(53, 0, 1, False) <= C.LDS_LIMIT < C.fwd_tile_lds_bytes(54, 0, 1, False)
    assert C.bwd_tile_lds_bytes(33, 33, 0, 1, False) > C.LDS_LIMIT


def test_tile_tables_exist_exactly_where_the_runs_say():
    for direction, runs in (("fwd", C.FORWARD_RUNS), ("rev", C.REVERSE_RUNS)):
        for name, (kw, pers) in runs.items():
            c = _case(direction, name)
            reverse = direction == "rev"
            sorted_col = bool(np.all(np.diff(c["send"] if reverse else c["recv"]) >= 0))
            assert sorted_col == (kw.get("order") != "shuffled"), (direction, name)
            for per in pers:
                tl = _table(c, per, reverse)
                assert tl is not None, (direction, name, per)
                lds = (C.bwd_tile_lds_bytes(tl["max_rows"], tl["max_own"], tl["max_edges"], c["B"]) if reverse else
                       C.fwd_tile_lds_bytes(tl["max_rows"], tl["max_edges"], c["B"]))
                assert lds <= C.LDS_LIMIT and tl["max_own"] <= C.TILE_NODES
                if per:
                    assert tl["max_own"] == min(per, int(np.diff(c["node_splits"]).max()))
            if not pers and c["B"] <= C.MAX_BASIS_TILES:
                assert _table(c, None, reverse) is None, (direction, name)
    # the route edges by name
    assert _table(_case("fwd", "complete49"), None, False) is not None and _table(_case("fwd", "complete50"), None, False) is None
    assert _table(_case("fwd", "complete48-b31"), None, False)["max_rows"] == 48
    assert _table(_case("rev", "complete50"), None, True) is not None                     # the mixed route
    assert _table(_case("rev", "complete56"), None, True) is not None and _table(_case("rev", "complete57"), None, True) is None
    for direction in ("fwd", "rev"):
        c = _case(direction, "trip-tiles")
        tl = _table(c, None, direction == "rev")
        assert c["G"] == 2100 and tl["count"] == 2100 > C.TILE_GRID and set(np.diff(c["node_splits"])) == {2, 3}
    assert _table(_case("fwd", "odd-47"), 62, False)["max_own"] == 47 and _table(_case("fwd", "steps"), 62, False) is None
    assert _table(_case("rev", "slots"), 62, True)["max_own"] == 16
    assert _table(_case("fwd", "odd"), 1, False) is None and _table(_case("rev", "odd"), 62, True) is None   # 63 rows of s and v


# ------------------------------------------------------------------------------------- degrees
def test_degree_lists():
    both = C.STEP_DEGREES + C.STEP_DEGREES[::-1]
    assert C.STEP_DEGREES == (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 0, 33, 16, 17)
    c = _case("fwd", "steps")
    assert c["N"] == 32 and tuple(T.in_degrees(c["edges"], 32, 0)) == both and c["M"] == sum(both) == 564
    pairs = [(both[i], both[i + 1]) for i in range(0, 32, 2)]
    assert any(min(p) <= 16 < max(p) for p in pairs) and any(min(p) <= 32 < max(p) for p in pairs)   # a step for one half only
    assert {(max(p) - 1) % 16 < 8 for p in pairs} == {True, False}                                   # the `bt` split, both ways
    r = _case("rev", "steps")
    assert tuple(T.in_degrees(r["edges"], 32, 1)) == both and np.all(np.diff(r["send"]) >= 0)
    s = _case("rev", "slots")
    assert C.SLOT_DEGREES == (1, 4, 5, 8, 9, 12, 13, 16, 17, 33)
    assert tuple(T.in_degrees(s["edges"], s["N"], 1)[3:13]) == C.SLOT_DEGREES and s["N"] == 19
    assert {min(d, 16) for d in C.SLOT_DEGREES} | {d - 16 for d in C.SLOT_DEGREES if d > 16} >= {1, 4, 5, 8, 9, 12, 13, 16}
    assert {(min(d, 16) + 3) >> 2 for d in C.SLOT_DEGREES} == {1, 2, 3, 4}                           # painn_bwd_slots<1..4>
    loops = s["recv"] == s["send"]
    assert loops.sum() == 1 and loops[-1] and s["dist"][-1] == 0 and not s["rij"][-1].any() and np.all(s["dist"][:-1] >= 0.9)
    assert np.all(np.isfinite(s["rbf"])) and np.all(np.isfinite(s["rbfd"]))
    for direction, col in (("fwd", 0), ("rev", 1)):
        g = _case(direction, "rounds")
        assert tuple(T.in_degrees(g["edges"], g["N"], col)[1:5]) == C.ROUND_DEGREES == (63, 64, 65, 130)
        assert {d % C.EC_FWD for d in C.ROUND_DEGREES} >= {7, 0, 1} and {d % C.EC_BWD for d in C.ROUND_DEGREES} >= {3, 0, 1, 2}
        assert max(C.ROUND_DEGREES) > 2 * C.GATHER_ROUND
        o = _case(direction, "odd")
        assert list(np.diff(o["node_splits"])) == [0, 1, 2, 3, 0, 5, 63, 0]
        w = _case(direction, "trip-waves")
        assert w["N"] == 8209 and 2 * w["N"] > C.GATHER_WAVES and w["M"] == 4105
        assert T.in_degrees(w["edges"], w["N"], col)[8192:].sum() == 9                               # the second trip has edges
    assert list(np.diff(_case("fwd", "odd-47")["node_splits"])) == [0, 1, 2, 3, 0, 5, 47, 0]
    sh = _case("fwd", "rounds-shuffled")
    assert np.any(np.diff(sh["recv"]) < 0) and np.any(np.diff(sh["send"]) < 0)
    assert _case("fwd", "rounds-b32-nobias")["B"] == 32 and _case("fwd", "rounds-b32-nobias")["bw"] is None
    assert _case("fwd", "steps-noresidual")["z_in"] is None and _case("fwd", "steps")["env"] is None
    assert {_case("fwd", "steps-b%d" % b)["B"] for b in (1, 7, 8)} == {1, 7, 8}


# ------------------------------------------------------------------------------------- restatements
@pytest.mark.parametrize("name", sorted(C.FORWARD_RUNS))
def test_message_forward_restatement(name):
    c = _case("fwd", name)
    assert c["s"].shape == (c["N"], 384) and c["v"].shape == (c["N"], 3, 128) and c["rbf"].shape == (c["M"], c["B"])
    (ds32, dv32), (ds64, dv64) = (C.message_forward_restate(c, dt) for dt in (np.float32, np.float64))
    assert np.all(np.isfinite(ds64)) and np.all(np.isfinite(dv64))
    silent = T.in_degrees(c["edges"], c["N"], 0) == 0
    if c["z_in"] is None:
        assert not ds64[silent].any() and not dv64[silent].any()
    else:
        assert np.array_equal(ds64[silent], c["z_in"][silent].astype(np.float64))
    _half_rows("message forward %s ds" % name, ds32, ds64)
    _half_rows("message forward %s dv" % name, dv32, dv64)


@pytest.mark.parametrize("name", sorted(C.REVERSE_RUNS))
def test_message_reverse_restatement(name):
    c = _case("rev", name)
    r32, r64 = (C.message_reverse_restate(c, dt) for dt in (np.float32, np.float64))
    assert r64["g_s"].shape == (c["N"], 384) and r64["g_d"].shape == (c["M"],) and r64["g_rij"].shape == (c["M"], 3)
    silent = T.in_degrees(c["edges"], c["N"], 1) == 0
    assert not r64["g_s"][silent].any() and np.array_equal(r64["g_v"][silent], c["g_dv"][silent].astype(np.float64))
    for k in ("g_s", "g_v"):
        _half_rows("message reverse %s %s" % (name, k), r32[k], r64[k])
    for k in ("g_d", "g_rij"):
        _half("message reverse %s %s" % (name, k), r32[k], r64[k], C.BAR_EDGE)


def test_message_reverse_restatement_is_the_derivative_along_the_distance():
    """Central differences in float64: moving every edge's distance by +-h changes ``rbf`` and the envelope (recomputed
    from the distance), and ``sum g_ds ds + sum g_dv dv`` by ``2 h sum g_d``, edge by edge."""
    c = C.message_case("slots", side="send", basis=7, seed=3)
    want = C.message_reverse_restate(c, np.float64)["g_d"]
    freq = np.pi * np.arange(1, 8, dtype=np.float32)
    h = 1e-6

    def edge_terms(d):
        cc = dict(c)
        cc["rbf"], _ = C.bessel_restate(d, freq, c["cutoff"], C.BESSEL["exponent"], np.float64)
        cc["env"], _ = C.cos_envelope_restate(d, c["cutoff"], np.float64)
        dt = torch.float64
        recv, send = (torch.from_numpy(c[k].astype(np.int64)) for k in ("recv", "send"))
        w = (C._tt(cc["rbf"], dt) @ C._tt(c["Ww"], dt) + C._tt(c["bw"], dt)) * C._tt(cc["env"], dt)[:, None]
        sw1, sw2, sw3 = torch.chunk(C._tt(c["s"], dt)[send] * w, 3, dim=-1)
        gz, gv = C._tt(c["g_ds"], dt)[recv], C._tt(c["g_dv"], dt)[recv]
        msg = sw2.unsqueeze(1) * C._tt(c["v"], dt)[send] + sw3.unsqueeze(1) * C._tt(c["rij"], dt).unsqueeze(-1)
        return ((gz * sw1).sum(-1) + (gv * msg).sum((-1, -2))).numpy()

    d = c["dist"].astype(np.float64)
    num = (edge_terms(d + h) - edge_terms(d - h)) / (2 * h)
    # (the stored basis rows are float32 roundings of the float64 basis: 6e-8 relative)
    assert np.max(np.abs(num - want)) <= 1e-6 * np.max(np.abs(want))


@pytest.mark.parametrize("name", sorted(C.geometry_cases()))
def test_geometry_cases(name):
    c = C.geometry_case(**C.geometry_cases()[name])
    e, n = c["edges"], c["N"]
    sorted0, sorted1 = bool(np.all(np.diff(e[:, 0]) >= 0)), bool(np.all(np.diff(e[:, 1]) >= 0))
    deg0, deg1 = T.in_degrees(e, n, 0), T.in_degrees(e, n, 1)
    if name.startswith("receiver-hubs"):
        assert sorted0 and not sorted1 and {64, 65, 100, 1000} <= set(deg0)
    if name == "sender-hubs":
        assert sorted1 and not sorted0 and {64, 65, 100, 1000} <= set(deg1)
    if name.startswith("shuffled"):
        assert not sorted0 and not sorted1
    if name.startswith("node-trip"):
        assert n == 8209 and sorted0 and not sorted1
    else:
        assert int(np.sum(e[:, 0] == e[:, 1])) == 8                                   # self loops: d = 0
    assert c["g_d"].shape == (c["slices"], c["M"]) and c["slices"] == (2 if name.endswith("two-slices") else 1)
    zero = c["dist"] == 0
    assert zero[c["coincident"]] and e[c["coincident"], 0] != e[c["coincident"], 1] and np.all(zero[e[:, 0] == e[:, 1]])
    r32, r64 = C.geometry_restate(c, np.float32), C.geometry_restate(c, np.float64)
    keep = dict(c, edges=e[~zero], dist=c["dist"][~zero], rij=c["rij"][~zero], g_d=c["g_d"][:, ~zero], g_rij=c["g_rij"][:, ~zero])
    assert np.array_equal(C.geometry_restate(keep, np.float64), r64)                  # a d = 0 edge changes no bit
    assert np.all(r64[(deg0 == 0) & (deg1 == 0)] == 0)
    assert np.max(np.abs(r64.sum(0))) <= 1e-9 * np.abs(r64).max()                     # actio = reactio
    _half("geometry %s (N %d, M %d)" % (name, n, c["M"]), r32, r64, C.BAR_FORCE)


@pytest.mark.parametrize("n,bias", C.UPDATE_RUNS)
def test_update_restatements(n, bias):
    c = C.update_case(n, bias=bias)
    assert (c["bd"] is None) == (c["ba"] is None) == (not bias) and c["uv"].shape == (3 * n, 256)
    f32, f64 = C.update_forward_restate(c, np.float32), C.update_forward_restate(c, np.float64)
    tag = "update N=%d%s" % (n, "" if bias else " no bias")
    assert np.array_equal(f64["c"][:, :128], c["zp"].astype(np.float64)) and np.all(f64["c"][:, 128:] > 0)
    for k in C.UPDATE_OUTPUTS:
        _half_rows("%s %s" % (tag, k), f32[k], f64[k])
    for with_g_v2 in (True, False):
        r32, r64 = (C.update_reverse_restate(c, dt, with_g_v2) for dt in (np.float32, np.float64))
        for k in ("g_zp", "g_uv"):
            _half_rows("%s reverse%s %s" % (tag, "" if with_g_v2 else " without g_v2", k), r32[k], r64[k])


@pytest.mark.parametrize("name", sorted(C.STAGE0_RUNS))
def test_stage0_cases(name):
    kw = C.STAGE0_RUNS[name]
    c = C.stage0_case(**kw)
    assert c["G"] == kw["graphs"] and (c["G"] > C.PREP_LDS_GRAPHS) == name.startswith("global")
    assert c["G"] in (1023, 1030) and set(c["sizes"]) == {1, 2, 3} and c["M"] == int(np.sum(c["sizes"] * (c["sizes"] - 1)))
    assert c["numbers"].dtype == (np.int64 if kw["numbers"] == "int64" else np.float32)
    r32, r64 = C.stage0_restate(c, np.float32), C.stage0_restate(c, np.float64)
    local = c["idx"]
    size = np.repeat(c["sizes"], np.diff(c["edge_splits"]))
    bad = ((local < 0) | (local >= size[:, None])).any(axis=1)
    assert np.array_equal(np.nonzero(bad)[0], c["marked"]) and len(c["marked"]) == (3 if kw.get("oob") else 0)
    graph_lo = np.repeat(c["node_splits"][:-1], np.diff(c["edge_splits"]))
    for k in ("recv", "send"):                                     # clamped into the edge's own graph
        assert np.all(r64[k] >= graph_lo) and np.all(r64[k] < graph_lo + size) and np.array_equal(r32[k], r64[k])
    assert np.all(r64["recv"] != r64["send"]) and r64["dist"].min() >= 0.9 - 1e-6
    far = r64["dist"] >= c["cutoff"]                               # edges beyond the Bessel cutoff: a zero basis row
    assert far.sum() == 6 and not r64["rbf"][far].any() and not r64["rbfd"][far].any() and not r32["rbf"][far].any()
    assert np.all(np.abs(r64["rbf"][~far]).max(axis=1) > 0)
    assert not r64["z0"][1].any() and not r64["z0"][c["N"] - 2].any() and np.abs(r64["z0"]).max(axis=1).min() == 0
    assert (r64["env"] is None) == (c["cos_cutoff"] <= 0)
    for k in ("dist", "rij", "rbf", "rbfd", "env", "envd", "z0", "v0"):
        if r64[k] is not None:
            _half_rows("stage 0 %s %s" % (name, k), r32[k], r64[k])


def test_stage0_basis_derivative_is_the_derivative():
    d = np.linspace(0.9, 4.9, 41)
    freq = np.pi * np.arange(1, 21, dtype=np.float32)
    h = 1e-6
    up, _ = C.bessel_restate(d + h, freq, 5.0, 5, np.float64)
    dn, _ = C.bessel_restate(d - h, freq, 5.0, 5, np.float64)
    _, want = C.bessel_restate(d, freq, 5.0, 5, np.float64)
    assert np.max(np.abs((up - dn) / (2 * h) - want)) <= 1e-7 * np.abs(want).max()
    (eu, _), (ed, _), (_, ew) = (C.cos_envelope_restate(x, 4.0, np.float64) for x in (d + h, d - h, d))
    assert np.max(np.abs((eu - ed) / (2 * h) - ew)) <= 1e-7 and not ew[d >= 4.0].any()


# ------------------------------------------------------------------------------------- composed batches
@pytest.mark.parametrize("name", sorted(C.MODEL_BATCHES))
def test_model_batches_and_the_float32_reference(name):
    b = C.model_batch(name, synth.radius_graph)
    ns, es = b["node_splits"], b["edge_splits"]
    sizes = np.diff(ns)
    assert np.array_equal(np.diff(es), sizes * (sizes - 1))                           # every molecule complete
    ptr0, perm0 = C.csr(np.concatenate([b["edge_indices"][es[g]:es[g + 1], 0] + ns[g] for g in range(len(sizes))]), int(ns[-1]))
    ptr1, _ = C.csr(np.concatenate([b["edge_indices"][es[g]:es[g + 1], 1] + ns[g] for g in range(len(sizes))]), int(ns[-1]))
    assert perm0 is None
    fwd, rev = message_tile_table(ns, ptr0, 20), message_tile_table(ns, ptr1, 20, reverse=True)
    if name == "tiles-both-ways":
        assert list(sizes) == [49, 21] and fwd is not None and rev is not None
    if name == "mixed-route":
        assert list(sizes) == [52, 21] and fwd is None and rev is not None
    if name == "trip-tiles":
        assert len(sizes) == 2100 and fwd["count"] > C.TILE_GRID and rev["count"] > C.TILE_GRID and int(ns[-1]) < 6400
    p = synth.painn_params(seed=8, random_bias=True)
    (e32, f32), (e64, f64) = (tfo.painn_energy_force(p, b, dt, equiv_method="eps", cutoff=None)
                              for dt in (torch.float32, torch.float64))
    print("[restatement] PaiNN model %s: float32 energies are %.2e from float64 (rowwise)" % (name, rowwise_rel(e32, e64)))
    worst = max(C.max_rel(f32[ns[g]:ns[g + 1]], f64[ns[g]:ns[g + 1]]) for g in range(len(sizes)))
    print("[restatement] PaiNN model %s: float32 forces at most %.2e of a molecule's scale from float64" % (name, worst))
    rows = max(rowwise_rel(f32[ns[g]:ns[g + 1]], f64[ns[g]:ns[g + 1]]) for g in range(len(sizes)))
    print("[restatement] PaiNN model %s: float32 atom rows at most %.2e from float64 (half bar %.1e)" % (name, rows, FORCE_RTOL / 2))
    assert rowwise_rel(e32, e64) <= RTOL / 2 and worst <= FORCE_RTOL / 2 and rows <= FORCE_RTOL / 2
    assert_forces_close(f32, f32, f64, ns, what="PaiNN model %s, float32 reference" % name)
