"""tests/schnet_node_cases.py on the CPU: the node counts reach what they claim (tiles, tiles per workgroup at each cap of
``launch_node_impl``, rows of the last tile - derived from the named constants, asserted per count); the float32
restatement of every case tests/test_gpu_schnet_node_edges.py compares - MID / LAST, the input chain, the layer-path
build - is at most half of ``BAR_CHAIN`` from its float64 twin in ``max_rel`` (a case that does not meet this is changed,
the bar stays; each figure is printed, the table in the GPU file's docstring is a copy); out-of-range and fractional node
numbers hit the embedding rows the docstrings say; the pack index formulas are permutations and the three-piece bf16
split is exact; the stage-0 cases lie on the intended side of ``tiles16 > 1024`` and ``G > 1023``."""
import numpy as np
import pytest

import schnet_node_cases as C


def _half(what, r32, r64):
    e = C.max_rel(r32, r64)
    print("[restatement] %s: float32 is %.2e of the largest magnitude from float64 (half bar %.1e)"
          % (what, e, C.BAR_CHAIN / 2))
    assert r32.dtype == np.float32 and r64.dtype == np.float64 and np.all(np.isfinite(r64))
    assert e <= C.BAR_CHAIN / 2, "%s: float32 restatement %.3g from float64, half bar %.3g" % (what, e, C.BAR_CHAIN / 2)
    return e


# ------------------------------------------------------------------------------------- A. MID and LAST
def test_flag_sets_select_the_four_grids():
    assert C.CHAIN_FLAGS == (2, 3, 66, 67, 66 | 512, 67 | 512)
    assert (C.TILE, C.CAP_FP32, C.CAP_BF, C.CAP_BF_HALF, C.HALF_FROM_TILES) == (16, 512, 256, 128, 256)
    for n in (1, 4080, 4081, 4097, 8193):
        assert C.cap_of(2, n) == C.cap_of(3, n) == 512 and C.cap_of(66, n) == C.cap_of(67, n) == 256
    assert C.cap_of(66 | 512, 4080) == 256 and C.cap_of(66 | 512, 4081) == 128 and C.cap_of(67 | 512, 4097) == 128
    assert C.cap_of(2 | 512, 8193) == 512                       # bit 9 means nothing to the FP32 builds


def test_node_counts_reach_the_tile_edges_and_every_trip():
    assert C.EDGE_COUNTS == (1, 15, 16, 17)
    assert [C.tiles(n) for n in C.EDGE_COUNTS] == [1, 1, 1, 2]
    assert [C.last_tile_rows(n) for n in C.EDGE_COUNTS] == [1, 15, 16, 1]
    assert (C.TRIP_FP32, C.TRIP_BF, C.HALF_FULL, C.HALF_TWO, C.HALF_THREE) == (8193, 4097, 4080, 4081, 4097)
    for flags in (2, 3):            # FP32: 513 tiles on 512 workgroups - workgroup 0 takes a second tile, of one row
        assert C.trip_counts(flags) == (8193,)
        assert C.tiles(8193) == 513 and C.grid_of(flags, 8193) == 512 and C.last_tile_rows(8193) == 1
        assert C.tiles_per_workgroup(flags, 8193) == (1, 2)
    for flags in (66, 67):          # bf16 pieces: 257 tiles on 256 workgroups
        assert C.trip_counts(flags) == (4097,)
        assert C.tiles(4097) == 257 and C.grid_of(flags, 4097) == 256 and C.tiles_per_workgroup(flags, 4097) == (1, 2)
        assert C.grid_of(flags, 4081) == 256 and C.tiles_per_workgroup(flags, 4081) == (1, 1)     # no trip without bit 9
    for flags in (66 | 512, 67 | 512):
        assert C.trip_counts(flags) == (4080, 4081, 4097)
        # 255 tiles: the full grid, one tile each, the last tile whole
        assert C.tiles(4080) == 255 and C.grid_of(flags, 4080) == 255 and C.last_tile_rows(4080) == 16
        assert C.tiles_per_workgroup(flags, 4080) == (1, 1)
        # 256 tiles on 128 workgroups: exactly two each, the last tile of one row
        assert C.tiles(4081) == 256 and C.grid_of(flags, 4081) == 128 and C.last_tile_rows(4081) == 1
        assert C.tiles_per_workgroup(flags, 4081) == (2, 2)
        # 257 tiles: workgroup 0 takes three
        assert C.tiles(4097) == 257 and C.grid_of(flags, 4097) == 128 and C.tiles_per_workgroup(flags, 4097) == (2, 3)
    for flags in C.CHAIN_FLAGS:
        runs = C.chain_runs(flags)
        assert len(set(runs)) == len(runs)
        assert {n for n, b, s in runs if b and not s} == set(C.chain_counts(flags))
        nobias = {n for n, b, s in runs if not b}
        assert 17 in nobias and any(C.tiles_per_workgroup(flags, n)[1] > 1 for n in nobias)
        assert [(n, b) for n, b, s in runs if s] == [(37, True)]
        for n in C.EDGE_COUNTS:     # small batches: one workgroup per tile whatever the flags
            assert C.grid_of(flags, n) == C.tiles(n)


ALL_CHAIN_RUNS = sorted({r for flags in C.CHAIN_FLAGS for r in C.chain_runs(flags)} | set(C.RESIDUAL_RUNS))


@pytest.mark.parametrize("n,bias,saturated", ALL_CHAIN_RUNS)
def test_chain_cases(n, bias, saturated):
    """The MID / LAST operands at every count of every flag set, and those of the layer-path build."""
    c = C.node_case(n, bias=bias, saturated=saturated)
    assert all((c[k] is None) == (not bias) for k in ("b2", "b3", "bl0", "bl1"))
    assert c["agg"].shape == c["n"].shape == (n, C.F) and c["Wl1"].shape == (C.F, C.H)
    r32, r64 = C.node_restate(c, np.float32), C.node_restate(c, np.float64)
    if saturated:
        assert r64["pre2"].max() > 20 and r64["pre2"].min() < -20 and r64["prel0"].max() > 20
    tag = "n=%d%s%s" % (n, "" if bias else " no bias", " saturated" if saturated else "")
    for k in ("n", "x", "h"):
        _half("MID / LAST %s %s" % (tag, k), r32[k], r64[k])
    assert np.array_equal(C.residual_restate(c, np.float64), r64["n"])
    if (n, bias, saturated) in C.RESIDUAL_RUNS:
        _half("layer path %s n_out" % tag, C.residual_restate(c, np.float32), C.residual_restate(c, np.float64))


def test_residual_runs():
    assert C.RESIDUAL_COUNTS == (1, 15, 16, 17, 8193)
    assert {n for n, b, s in C.RESIDUAL_RUNS if b and not s} == set(C.RESIDUAL_COUNTS)
    assert {n for n, b, s in C.RESIDUAL_RUNS if not b} == {17, 8193} and (37, True, True) in C.RESIDUAL_RUNS
    assert C.tiles_per_workgroup(0, 8193) == (1, 2)             # NODE_UPD is an FP32 build


# ------------------------------------------------------------------------------------- B. input chain
def test_input_chain_runs_cover_the_counts_and_patterns():
    assert C.IN_FLAGS == (2, 3, 66, 67, 67 | 512)
    assert C.in_counts(2) == C.in_counts(3) == (1, 15, 16, 17, 33, 8193)
    assert C.in_counts(66) == C.in_counts(67) == (1, 15, 16, 17, 33, 4097)
    assert C.in_counts(67 | 512) == (1, 15, 16, 17, 33, 4097, 4081)
    for flags in C.IN_FLAGS:
        for i64 in (False, True):
            runs = C.in_runs(flags, i64)
            assert len(set(runs)) == len(runs)
            assert {n for n, p, v in runs if p == "uniform" and v == C.VOCAB} == set(C.in_counts(flags))
            want = set(C.IN_PATTERNS) - ({"fractional"} if i64 else set())
            assert {p for n, p, v in runs if n == 17 and v == C.VOCAB} == want
            assert {p for n, p, v in runs if n == 33 and v == C.VOCAB} == want
            last = {n for n, p, v in runs if p == "oob-last" and v == C.VOCAB}
            # the out-of-range row is the only row of a tile taken on a second trip, the last row of a whole tile, and
            # the last row of a partial one
            assert any(C.last_tile_rows(n) == 1 and C.tiles_per_workgroup(flags, n)[1] == 2 for n in last)
            assert 16 in last and 17 in last and 33 in last
            assert {v for n, p, v in runs} == {C.VOCAB, 1}


@pytest.mark.parametrize("i64", [False, True])
@pytest.mark.parametrize("emb_dim", [64, 128])
def test_input_chain_cases(emb_dim, i64):
    """Every run of every build (the numbers do not depend on the flags): the rows hit, and the float32 restatement."""
    runs = sorted({r for flags in C.IN_FLAGS for r in C.in_runs(flags, i64)})
    zero_rows = truncated = 0
    worst = 0.0
    for bias in (True, False):
        for n, pattern, vocab in runs:
            c = C.in_case(n, emb_dim, pattern, vocab, bias=bias, i64=i64)
            num = c["numbers"]
            assert num.shape == (n,) and num.dtype == (np.int64 if i64 else np.float32)
            assert c["emb"].shape == (vocab, emb_dim) and c["W0"].shape == (emb_dim, C.F) and (c["b0"] is None) == (not bias)
            z, valid = C.in_rows(c)
            if pattern in ("uniform", "same", "ends", "fractional"):
                assert valid.all()
            if pattern == "same":
                assert len(set(z)) == 1
            if pattern == "ends" and n > 1:
                assert set(z) == {0, vocab - 1}
            if pattern == "oob":
                bad = {int(v) for v in num[~valid]}
                assert bad <= {-1, vocab, 1000, 2 ** 31 + 3} and (n < 17 or {-1, vocab, 1000} <= bad)
                assert not valid[2 % n] and (n < 3 or valid[:2].all())
                if i64 and n >= 33:
                    assert 2 ** 31 + 3 in bad and z[num == 2 ** 31 + 3][0] < 0             # wraps to a negative int32
            if pattern == "fractional":
                frac = num != np.trunc(num)
                assert {float(v) for v in num[frac]} == {float(np.float32(v)) for v in C.FRACTIONS}
                assert {int(v) for v in z[frac]} == {5, 94, 0} and np.all(z[num == np.float32(-0.5)] == 0)
                truncated += int(frac.sum())
            if pattern == "oob-last":
                assert not valid[-1] and valid[:-1].all() and num[-1] == vocab
            if pattern == "oob-first":
                assert not valid[0] and valid[1:].all() and num[0] == -1
            r32, r64 = C.in_restate(c, np.float32), C.in_restate(c, np.float64)
            if (~valid).any():                  # a zero embedding row: n = b0 exactly, and 0 without a bias
                zero_rows += int((~valid).sum())
                want = np.zeros(C.F) if c["b0"] is None else c["b0"].astype(np.float64)
                assert np.all(r64["n"][~valid] == want[None, :]) and np.all(r32["n"][~valid] == want.astype(np.float32))
                if c["b0"] is None:
                    assert not r64["x"][~valid].any()
            if valid.any():
                assert np.abs(r64["n"][valid]).max() > 0.5                              # real embedding rows set the scale
            for k in ("n", "x"):
                if np.abs(r64[k]).max() == 0:   # (every row out of range, no bias)
                    assert not r32[k].any()
                    continue
                tag = "input chain E=%d %s n=%d %s vocab=%d%s %s" % (emb_dim, "int64" if i64 else "float32", n, pattern,
                                                                    vocab, "" if bias else " no bias", k)
                worst = max(worst, _half(tag, r32[k], r64[k]))
    print("[restatement] input chain E=%d %s: at most %.2e over %d runs" % (emb_dim, "int64" if i64 else "float32", worst,
                                                                           2 * len(runs)))
    assert zero_rows > 0 and (i64 or truncated > 0)


def test_a_changed_embedding_row_shows_in_the_restatement():
    c = C.in_case(17, 64, "oob-last")
    r = C.in_restate(c, np.float64)
    c["emb"] = c["emb"] + 1.0
    r2 = C.in_restate(c, np.float64)
    assert np.array_equal(r["n"][-1], r2["n"][-1]) and not np.allclose(r["n"][:-1], r2["n"][:-1])


# ------------------------------------------------------------------------------------- C. stage 0
def test_stage0_cases_lie_on_the_intended_side_of_every_threshold():
    assert (C.STAGE0_MAX_TILES, C.STAGE0_MAX_GRAPHS) == (1024, 1023)
    seen = {}
    for name, (build, fused) in C.stage0_cases().items():
        b = build()
        n, m, g = len(b["node_number"]), len(b["edge_indices"]), len(b["node_splits"]) - 1
        seen[name] = (n, m, g)
        assert C.stage0_fused(n, m, g) == fused, name
        assert b["node_splits"][-1] == n and b["edge_splits"][-1] == m and len(b["edge_splits"]) == g + 1
        assert b["node_coordinates"].shape == (n, 3) and b["edge_indices"].dtype == np.int64
        sizes = np.diff(b["node_splits"])
        for k in range(g):                      # local ids inside the graph, receivers in order
            e = b["edge_indices"][b["edge_splits"][k]:b["edge_splits"][k + 1]]
            assert len(e) == 0 or (e.min() >= 0 and e.max() < sizes[k] and np.all(np.diff(e[:, 0]) >= 0))
    assert seen["tiles-1024"][0] == 16384 and C.tiles(16384) == 1024 and seen["tiles-1025"][0] == 16385
    assert C.tiles(16385) == 1025 > C.STAGE0_MAX_TILES and seen["tiles-1024"][1:] == seen["tiles-1025"][1:]
    assert seen["graphs-1023"] == (1023, 1023, 1023) and seen["graphs-1024"] == (1024, 1024, 1024)
    assert seen["no-edges"][1] == 0 and seen["no-edges"][0] > 0 and seen["no-nodes"][:2] == (0, 0)
    n, m, g = seen["second-tile"]
    assert n == C.TRIP_BF and 200 <= m <= 400 and C.tiles_per_workgroup(67, n) == (1, 2) and C.grid_of(3, n) == C.tiles(n)
    n, m, g = seen["second-tile-half-grid"]
    assert n == C.HALF_TWO and C.tiles_per_workgroup(67 | 512, n) == (2, 2) and C.tiles_per_workgroup(67, n) == (1, 1)
    # the eight-wave launch: half the edge workgroups, 64 at most - reached from 129 workgroups of 256 edges on
    assert C.stage0_edge_blocks_bf(300) == (1, 1) and C.stage0_edge_blocks_bf(128 * 256) == (64, 64)
    assert C.stage0_edge_blocks_bf(128 * 256 + 1) == (65, 64)
    # self edges only in the single-node graphs
    b = C.stage0_cases()["graphs-1023"][0]()
    assert not b["edge_indices"].any()


# ------------------------------------------------------------------------------------- E. pack kernels
@pytest.mark.parametrize("k,u", C.PACK_SHAPES)
def test_pack_formulas_are_permutations_and_the_split_is_exact(k, u):
    w = C.pack_weights(k, u)
    mag = np.abs(w[w != 0])
    assert w.shape == (k, u) and (w == 0).sum() >= k * u // 17 and (w > 0).any() and (w < 0).any()
    assert mag.max() / mag.min() > 1e6
    rows, cols = C.pack_index(k, u)
    assert len(rows) == k * u and len(np.unique(rows * u + cols)) == k * u          # a permutation of W
    assert rows.min() == 0 and rows.max() == k - 1 and cols.min() == 0 and cols.max() == u - 1
    assert np.array_equal(np.sort(C.pack_restate(w)), np.sort(w.reshape(-1)))
    # the first float4 of the image: k = 0, 4, 8, 12 of column 0; lane 16 holds k = 1
    assert list(rows[:4]) == [0, 4, 8, 12] and list(cols[:4]) == [0] * 4 and rows[64] == 1 and cols[4] == 1
    pc, rows, cols = C.pack_bf16_index(k, u)
    assert len(pc) == 3 * k * u and len(np.unique((pc * k + rows) * u + cols)) == 3 * k * u
    assert list(rows[:8]) == list(range(8)) and set(pc[:512]) == {0} and set(pc[512:1024]) == {1}
    bits, values = C.bf16_split(w)
    assert bits.shape == values.shape == (3, k, u) and bits.dtype == np.uint16
    total = values[0].astype(np.float64) + values[1].astype(np.float64) + values[2].astype(np.float64)
    assert np.array_equal(total, w.astype(np.float64))                              # hi + mid + lo == W, every element
    assert np.abs(values[1]).max() > 0 and np.abs(values[2]).max() > 0
    assert np.all(np.abs(values[1]) <= np.abs(values[0]) * 2.0 ** -8) and np.all(np.abs(values[2]) <= np.abs(values[0]) * 2.0 ** -16)
    assert np.array_equal((bits[0].astype(np.uint32) << 16).view(np.float32), values[0])
    halves = C.pack_bf16_restate(w)
    assert np.array_equal(C.pack_bf16_decode(halves, k, u), values)
