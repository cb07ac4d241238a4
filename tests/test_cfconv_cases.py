"""tests/cfconv_cases.py on the CPU: the layout graphs reach every wave-uniform tile shape the segment walk of
csrc/mp_cfconv.hip branches on, the edge counts give the tile, grid and trip numbers they claim (dispatch arithmetic
restated here), the restatement agrees with the project's oracle, and on every case tests/test_gpu_cfconv_edges.py
compares, the float32 restatement is at most half of ``parity.RTOL`` from its float64 twin in ``parity.rowwise_rel`` (the
engine may be as far from the float32 restatement as that one is from float64; a case that does not meet this is
changed, the bar stays).  Each figure is printed; the table in the GPU file's docstring is a copy."""
import numpy as np
import pytest

import cfconv_cases as C
import topologies as T
from oracle import kgcnn_oracle as ko
from parity import BAR_CAP, RTOL, rowwise_rel


def _edges(c):
    return np.stack([c["recv"], c["send"]], axis=-1).astype(np.int64)


def _half_rows(what, r32, r64):
    """assert_rows_close with the float64 twin: the bar is max(RTOL, min(2 x this distance, BAR_CAP)).  Held to RTOL / 2
    here: the bar then stays at RTOL."""
    e = rowwise_rel(r32, r64)
    print("[restatement] %s: float32 rows are %.2e from float64 (half bar %.1e)" % (what, e, RTOL / 2))
    assert e <= RTOL / 2 <= BAR_CAP / 2, "%s: float32 restatement %.3g from float64" % (what, e)
    return e


# ------------------------------------------------------------------------------------------------ A, B, G: layouts
def _features(recv_sorted):
    """(class, property) pairs of a sorted receiver list: class = (nlo > 1, cont, nhi > 1); properties: "tile", the first
    segment continues from the previous tile ("prev"), the last one into the next ("next"), the low / high half has exactly
    one opening ("lo1" / "hi1": its first segment is kept, nothing stored) or two and more ("lo2" / "hi2": a segment that
    closes after another one opened there is stored)."""
    out = {}
    for s in C.tile_shapes(recv_sorted):
        k = C.shape_class(s)
        props = ["tile"] + ["prev"] * bool(s["from_prev"]) + ["next"] * bool(s["into_next"])
        props += ["lo1"] * (s["open_lo"] == 1) + ["lo2"] * (s["open_lo"] >= 2)
        props += ["hi1"] * (s["open_hi"] == 1) + ["hi2"] * (s["open_hi"] >= 2)
        for p in props:
            out[(k, p)] = out.get((k, p), 0) + 1
    return out


def test_layout_graph_places_boundaries_at_every_edge_of_a_tile():
    c = C.get("layout")
    pats = C.layout_patterns()
    assert len(pats) == len(C.FIXED_PATTERNS) + C.RANDOM_PATTERNS == 80 and all(sum(p) == C.TILE == T.TILE for p in pats)
    assert c["M"] == 80 * 32 and np.all(np.diff(c["recv"]) >= 0) and C.kernel_order(c)[1] is None
    masks = [int(v) for v in C.start_masks(c["recv"])]
    assert masks[0] == 0                                                      # one receiver owns the tile
    assert masks[1:32] == [1 << k for k in range(1, 32)]                      # one boundary, at edge 1 .. 31
    named = dict(zip(("ones", "twos", "16|16", "15,1,1,15", "15,2,15", "1,30,1", "8x4", "1,14,1,1,14,1"), masks[32:40]))
    assert named["ones"] == 0xfffffffe                                        # 32 single-edge receivers
    assert named["twos"] == 0x55555554
    assert named["16|16"] == 1 << 16
    assert named["15,1,1,15"] == (1 << 15) | (1 << 16) | (1 << 17)
    assert named["15,2,15"] == (1 << 15) | (1 << 17)                          # an interior segment over edges 15|16
    assert named["1,30,1"] == (1 << 1) | (1 << 31)
    assert named["8x4"] == (1 << 8) | (1 << 16) | (1 << 24)
    assert named["1,14,1,1,14,1"] == (1 << 1) | (1 << 15) | (1 << 16) | (1 << 17) | (1 << 31)
    straddle = [s for s in C.tile_shapes(c["recv"]) if s["cont"] and s["nlo"] > 1 and s["nhi"] > 1]
    assert len(straddle) >= 10                                                # store_row(node_e16, ...) of low tail + high first
    place = T.tile_placement(_edges(c), c["N"])
    assert place["max_tiles_touched"] == 1 <= 2 and place["starts_on_boundary"] >= 80 and place["ends_on_boundary"] >= 80
    deg = T.in_degrees(_edges(c), c["N"])
    assert deg[0] == 0 and deg[-1] == 0 and int(np.sum(deg[1:-1] == 0)) >= 40    # receivers without edges in between
    assert [int(d) for d in deg[:len(C.layout_degrees())]] == C.layout_degrees()
    loops = c["recv"] == c["send"]
    assert int(loops.sum()) == 80 and np.all(loops.reshape(80, 32).sum(axis=1) == 1)     # one self loop per pattern
    assert np.array_equal(c["dist"] == 0, loops)
    same = (c["recv"][1:] == c["recv"][:-1]) & (c["send"][1:] == c["send"][:-1])
    assert int(np.sum(np.add.reduceat(same, np.arange(0, c["M"] - 1, 32)) > 0)) >= 75    # a duplicated sender per pattern


def test_unaligned_graph_lets_segments_run_across_tiles():
    c = C.get("unaligned")
    deg = T.in_degrees(_edges(c), c["N"])
    assert set(deg[deg > 0]) == set(C.UNALIGNED_DEGREES) | {1000} and int(np.sum(deg == 1000)) == 1
    assert deg[0] == 0 and deg[-1] == 0 and np.all(deg[1:-1] > 0) and C.kernel_order(c)[1] is None
    place = T.tile_placement(_edges(c), c["N"])
    assert place["max_whole_tiles"] >= 30 and place["max_tiles_touched"] >= 32      # a receiver owns 30 whole tiles
    shapes = C.tile_shapes(c["recv"])
    assert sum(s["from_prev"] for s in shapes) > len(shapes) // 2
    t = C.get("bins20")                                                        # the trimmed graph: its first 400 edges
    assert t["M"] == 400 and t["N"] == c["N"] and np.array_equal(t["recv"], c["recv"][:400])
    assert int(np.sum(T.in_degrees(_edges(t), t["N"]) == 0)) > 500


def test_layout_and_unaligned_graphs_reach_every_tile_shape():
    fa, fb = _features(C.get("layout")["recv"]), _features(C.get("unaligned")["recv"])
    both = {k: fa.get(k, 0) + fb.get(k, 0) for k in set(fa) | set(fb)}
    classes = [(a, b, d) for a in (False, True) for b in (False, True) for d in (False, True)]
    for k in classes:
        tag = "nlo %s, %s, nhi %s" % (">1" if k[0] else "=1", "cont" if k[1] else "edge 16 opens", ">1" if k[2] else "=1")
        row = {p: both.get((k, p), 0) for p in ("tile", "prev", "next", "lo1", "lo2", "hi1", "hi2")}
        print("[layout] %-34s aligned %3d, unaligned %3d tiles; %s" % (tag, fa.get((k, "tile"), 0), fb.get((k, "tile"), 0),
                                                                       row))
        assert row["tile"] > 0, tag
        assert row["prev"] > 0 and row["next"] > 0, tag       # its first / last segment continues in the neighbour tile
        # with and without a second opening in the same half (a half of one segment has no opening at all)
        assert (row["lo1"] > 0 and row["lo2"] > 0) if k[0] else (row["lo1"] == row["lo2"] == 0), tag
        assert (row["hi1"] > 0 and row["hi2"] > 0) if k[2] else (row["hi1"] == row["hi2"] == 0), tag
    assert not any(p in ("prev", "next") for (_, p) in fa)                     # the aligned graph has no continuation


@pytest.mark.parametrize("name", ["layout", "unaligned"])
def test_shuffled_graphs_hold_the_same_edges_in_another_order(name):
    c, s = C.get(name), C.get(name + "-shuffled")
    assert s["M"] == c["M"] and s["N"] == c["N"] and not np.all(np.diff(s["recv"]) >= 0)
    a, b = _edges(c), _edges(s)
    assert np.array_equal(a[np.lexsort((a[:, 1], a[:, 0]))], b[np.lexsort((b[:, 1], b[:, 0]))])
    recv_sorted, perm = C.kernel_order(s)
    assert perm is not None and perm.dtype == np.int32 and np.array_equal(np.sort(perm), np.arange(s["M"]))
    assert np.all(np.diff(recv_sorted) >= 0) and np.array_equal(recv_sorted, c["recv"])
    inside = recv_sorted[1:] == recv_sorted[:-1]
    assert np.all(np.diff(perm.astype(np.int64))[inside] > 0)                  # list order inside every receiver
    assert [x["mask"] for x in C.tile_shapes(recv_sorted)] == [x["mask"] for x in C.tile_shapes(c["recv"])]


# ------------------------------------------------------------------------------------------------ C, D: counts, grids, trips
def dispatch(m, bins, flags):
    """``cfconv_dispatch`` of csrc/mp_cfconv.hip restated: tiles, waves per workgroup, workgroups, trips of the
    persistent tile loop."""
    ntiles = -(-m // 32)
    waves = 4
    if ntiles >= 3072:
        waves = 8 if 37 * (-(-ntiles // 2048)) < 20 * (-(-ntiles // 1024)) else 4
    if flags & 4:
        waves = 8
    if flags & 8:
        waves = 4
    if not (flags & 1 and bins in (20, 25)):
        waves = 4
    grid = -(-ntiles // waves)
    if flags & 16 and grid > 1:
        grid = (grid + 1) // 2
    grid = min(grid, 256)
    return {"ntiles": ntiles, "waves": waves, "grid": grid, "trips": -(-ntiles // (grid * waves))}


def test_edge_counts_grids_and_trips():
    assert C.EXACT_COUNTS == (1, 31, 32, 33, 127, 128, 129, 255, 256, 257)
    want_tiles = {1: 1, 31: 1, 32: 1, 33: 2, 127: 4, 128: 4, 129: 5, 255: 8, 256: 8, 257: 9}
    for m in C.EXACT_COUNTS:
        c = C.get("exact%d" % m)
        assert c["M"] == m and c["N"] == 5 and np.all(np.diff(c["recv"]) >= 0)
        d1, d5, d17 = (dispatch(m, 20, f) for f in (1, 5, 17))
        assert d1["ntiles"] == want_tiles[m] and d1["waves"] == 4 and d5["waves"] == 8 and d17["waves"] == 4
        assert d1["grid"] == -(-want_tiles[m] // 4) and d1["trips"] == 1 and d5["grid"] == 1 + (m > 256)
        assert (d1["grid"] * 4 > d1["ntiles"]) == (m in (1, 31, 32, 33, 129, 257))      # waves without a tile
    grids = []
    for g in C.SWEEP_GROUPS:
        c = C.get("sweep%d" % g)
        assert c["M"] == 128 * g - 5 and c["M"] % 32 == 27
        d1, d5, d17 = (dispatch(c["M"], 20, f) for f in (1, 5, 17))
        assert d1["ntiles"] == 4 * g and d1["grid"] == g and d1["trips"] == 1
        assert d5["grid"] == (g + 1) // 2 and d17["grid"] == ((g + 1) // 2 if g > 1 else 1) and d17["trips"] == (2 if g > 1 else 1)
        grids.append(d1["grid"])
    assert grids == list(range(1, 18)) and {g % 8 for g in grids} == set(range(8))     # every remainder of the XCD order
    t4, t8 = C.get("trip4"), C.get("trip8")
    assert t4["M"] == 32 * 1024 + 33 == 32801 and t4["N"] == 40 and t8["M"] == 32 * 2048 + 33 == 65569
    d = dispatch(t4["M"], 20, 1)
    assert d == {"ntiles": 1026, "waves": 4, "grid": 256, "trips": 2} and t4["M"] > 32768
    assert d["ntiles"] - 256 * 4 == 2 and t4["M"] % 32 == 1            # the second trip: one whole tile, one of one edge
    assert dispatch(t4["M"], 20, 5) == {"ntiles": 1026, "waves": 8, "grid": 129, "trips": 1}
    assert dispatch(t4["M"], 20, 17) == {"ntiles": 1026, "waves": 4, "grid": 129, "trips": 2}
    assert dispatch(t4["M"], 20, 33) == dispatch(t4["M"], 20, 1)
    d = dispatch(t8["M"], 20, 5)
    assert d == {"ntiles": 2050, "waves": 8, "grid": 256, "trips": 2} and d["ntiles"] - 256 * 8 == 2 and t8["M"] > 65536
    assert dispatch(t8["M"], 20, 33) == {"ntiles": 2050, "waves": 4, "grid": 256, "trips": 3}
    for c, wave_tiles in ((t4, 1024), (t8, 2048)):
        # one receiver owns the last whole tile of the first trip and the first of the second
        lo, hi = 32 * (wave_tiles - 1), 32 * (wave_tiles + 1) - 1
        assert c["recv"][lo] == c["recv"][hi] and np.all(np.diff(c["recv"]) >= 0)
        assert T.tile_placement(_edges(c), c["N"])["max_whole_tiles"] >= 20
    assert dispatch(257, 20, 17) == {"ntiles": 9, "waves": 4, "grid": 2, "trips": 2}
    assert dispatch(1333, 20, 17) == {"ntiles": 42, "waves": 4, "grid": 6, "trips": 2}
    assert C.get("half257")["M"] == 257 and C.get("half1333")["M"] == 1333 and C.get("half1333")["N"] == 40
    assert dispatch(400, 24, 5)["waves"] == 4 and dispatch(400, 25, 5)["waves"] == 8 and dispatch(400, 20, 4)["waves"] == 4


# ------------------------------------------------------------------------------------------------ E, F: bases, parameters
def test_basis_sizes_sit_on_either_side_of_the_fixed_builds():
    assert C.BASES == (1, 2, 19, 20, 21, 24, 25, 26, 30, 31, 32)
    nk = {b: (b + 2) >> 1 for b in C.BASES}
    assert nk == {1: 1, 2: 2, 19: 10, 20: 11, 21: 11, 24: 13, 25: 13, 26: 14, 30: 16, 31: 16, 32: 17}
    assert [b for b in range(1, C.MAX_BINS + 1) if (b + 2) >> 1 > C.G1B_MAX_NK] == [32]    # zeros in the bf16 image of W1
    assert {b for b in C.BASES if 2 * nk[b] > b + 1} == {2, 20, 24, 26, 30, 32}            # B + 1 rows odd: a zero padding row
    for b in C.BASES:
        c = C.get("bins%d" % b)
        assert c["bins"] == b and c["w1"].shape == (b, C.F) and C.given_rbf(c).shape == (400, b)
        assert C.given_rbf(c).dtype == np.float32


@pytest.mark.parametrize("name", C.PARAMETER_CASES + C.LAYER_CASES)
def test_parameter_cases(name):
    c = C.get(name)
    assert all(np.float32(c[k]) == c[k] for k in ("distance", "sigma", "offset"))
    assert (c["b1"] is None) == (name in ("no-b1", "no-bias", "layer-no-bias"))
    assert (c["b2"] is None) == (name in ("no-b2", "no-bias", "layer-no-bias"))
    ordinary = np.setdiff1d(np.arange(c["M"]), c["marked"])
    pre = C.pre1_of(c)
    if name == "offset":
        assert c["offset"] == 0.75
    if name == "sigma0.1-bins32":
        assert c["sigma"] == float(np.float32(0.1)) and c["bins"] == 32
    if name == "d-zero":
        assert len(c["marked"]) == 8 and np.all(c["dist"][c["marked"]] == 0) and np.all(c["dist"][ordinary] > 0)
    if name == "d-far":
        assert np.all(c["dist"][c["marked"]] == np.float32(15.0)) and c["dist"][ordinary].max() < 10
        assert C.gauss_rbf(c, np.float64)[c["marked"]].max() < 1e-100         # far outside the basis: the filter of b1 alone
    if name == "saturated":
        assert abs(np.abs(pre).max() - C.SATURATED_PRE) < 0.5 and (pre > 50).any() and (pre < -50).any()
    else:
        assert np.abs(pre).max() < 10
    if name == "layer-det":
        deg = T.in_degrees(_edges(c), c["N"])
        assert c["bins"] == 25 and deg.max() == 1000 and int(np.sum(deg > 32)) > 100 and C.kernel_order(c)[1] is not None


# ------------------------------------------------------------------------------------------------ restatement
def test_restatement_against_the_oracle():
    """``cfconv_restate`` against oracle.kgcnn_oracle (``gauss_basis`` + ``schnet_cfconv``) on a default case: the
    restatement is not its own witness."""
    c = C.get("bins20")
    ns, es = np.array([0, c["N"]], np.int64), np.array([0, c["M"]], np.int64)
    for dt, bar in ((np.float64, 1e-12), (np.float32, RTOL / 2)):
        rbf = ko.gauss_basis(ko.R(c["dist"].astype(dt).reshape(-1, 1), es), c["bins"], c["distance"], c["sigma"], c["offset"])
        assert rowwise_rel(rbf.values, C.gauss_rbf(c, np.float64)) <= (1e-12 if dt is np.float64 else 2e-6)
        p = ko.to_dtype({"dense1/kernel": c["w1"], "dense1/bias": c["b1"], "dense2/kernel": c["w2"], "dense2/bias": c["b2"]},
                        dt)
        want = ko.schnet_cfconv(ko.R(c["x"].astype(dt), ns), rbf, ko.R(_edges(c), es), p).values
        e = rowwise_rel(C.cfconv_restate(c, dt), want)
        print("[restatement] against the oracle in %s: %.2e" % (np.dtype(dt).name, e))
        assert e <= bar
        e = rowwise_rel(C.cfconv_restate(c, dt, rbf=rbf.values), want)        # and from a given basis matrix
        assert e <= bar


@pytest.mark.parametrize("name", sorted(C.cases()))
def test_float32_restatement_is_within_half_the_bar(name):
    c = C.get(name)
    r32, r64 = C.restated(name)
    assert r32.dtype == np.float32 and r64.dtype == np.float64 and r64.shape == (c["N"], C.F) and np.all(np.isfinite(r64))
    deg = T.in_degrees(_edges(c), c["N"])
    assert not r64[deg == 0].any() and np.all(np.abs(r64[deg > 0]).max(axis=1) > 0)
    _half_rows("%s (N %d, M %d, bins %d)" % (name, c["N"], c["M"], c["bins"]), r32, r64)
    if name in C.BASIS_CASES + C.LAYER_CASES:                                  # (the layer takes a basis matrix)
        g32, g64 = C.restated(name, "rbf")
        _half_rows("%s from a given basis matrix" % name, g32, g64)
        assert rowwise_rel(g64, r64) <= 1e-6                                   # the matrix is the basis rounded to float32


def test_pack_image_decoders_cover_every_entry():
    ones = lambda k: np.full(k, 0x3f803f80, np.uint32).view(np.float32)     # two bf16 ones per slot
    image = ones(3 * C.W2_PIECE_FLOATS)
    assert not np.isnan(C.decode_w2_images(image)).any()                      # every (piece, row, column) is written
    for bins in (1, 20, 31):
        nk = (bins + 2) >> 1
        w1, unused = C.decode_w1_images(ones(C.W1B_FLOATS), bins)
        assert np.all(w1[:, :2 * nk] != 0) and not w1[:, 2 * nk:].any() and (unused != 0) == (nk < 16)
    assert C.PACKED_FLOATS == 34 * 128 + 3 * 8192 + 128 + 6144
    assert C.rowmap(5, 1) == 1 + 8 + 4 and sorted(C.rowmap(r, h) for r in range(16) for h in (0, 1)) == list(range(32))
