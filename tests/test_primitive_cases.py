"""tests/primitive_cases.py on the CPU: every generator delivers the boundary it claims (segment lengths and rounds, work
items against the 524 288-thread grid cap, graph counts around the LDS search, the chunk plan of the weight gradient, the
tile table and the edge windows of the GCN tile kernel), and on every case tests/test_gpu_primitive_edges.py compares in
floating point, the float32 restatement is inside half the cap that test applies (the engine may be as far from the
float32 restatement as that one is from float64; a case that does not meet this is shrunk, the cap stays).  Each distance
is printed; the table in the GPU file's docstring is a copy of this output."""
import numpy as np
import pytest

import primitive_cases as P
from oracle import kgcnn_oracle as ko
from parity import BAR_CAP, rowwise_rel

MEAN_RTOL = 1e-6        # tests/test_gpu_layers.py::test_pooling_local_edges, mean
WEIGHTED_RTOL = 2e-6    # tests/test_gpu_layers.py::test_pooling_weighted_local_edges


def _half(what, r32, r64, cap=BAR_CAP):
    e = rowwise_rel(r32, r64)
    print("[restatement] %s: float32 is %.2e from float64 (half cap %.1e)" % (what, e, cap / 2))
    assert e < cap / 2, "%s: float32 restatement %.3g from float64, half cap %.3g" % (what, e, cap / 2)
    return e


# ----------------------------------------------------------------------------------------------------- activations
def test_activation_restatements_agree_with_the_oracle_and_their_derivatives():
    x = np.linspace(-6, 6, 241)
    for code, name in P.ACT_NAMES.items():
        assert np.allclose(P.act(code, x), ko.activation(name, x), rtol=1e-12, atol=1e-12), name
        assert P.act(code, x.astype(np.float32)).dtype == np.float32
        assert P.act_grad(code, x.astype(np.float32)).dtype == np.float32
        h = 1e-6
        xs = x[np.abs(x) > 1e-3]                       # relu, leaky_relu and selu have a kink at 0
        num = (P.act(code, xs + h) - P.act(code, xs - h)) / (2 * h)
        assert np.allclose(P.act_grad(code, xs), num, rtol=1e-6, atol=1e-8), name


# --------------------------------------------------------------------------------------------------- A. segments
def test_segment_lengths_reach_every_round_shape():
    L = P.SEGMENT_LENGTHS
    assert L == (0, 1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 0, 129, 1000, 0)
    assert L[0] == 0 and L[-1] == 0 and 0 in L[1:-1]
    shapes = {n: P.rounds_of(n) for n in L}
    assert shapes[15] == (0, 2, 7) and shapes[16] == (1, 0, 16) and shapes[17] == (1, 1, 1) and shapes[31] == (1, 2, 7)
    assert shapes[33] == (2, 1, 1) and shapes[129] == (8, 1, 1) and shapes[1000] == (62, 1, 8)
    assert {s[2] for n, s in shapes.items() if n} >= {1, 7, 8, 16}          # rows of the last, partial round
    assert any(s[0] and s[1] == 2 for s in shapes.values())                 # a 16-row round, then two 8-row rounds
    assert P.SEGMENT_WIDTHS == (1, 3, 4, 128, 130) and L[P.ZERO_WEIGHT_SEGMENT] == 8
    ptr = P.segment_ptr()
    assert ptr.dtype == np.int32 and ptr[-1] == sum(L) and np.array_equal(np.diff(ptr), L)


@pytest.mark.parametrize("perm", [False, True])
@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("weight", [False, True])
def test_segment_case_operands(perm, gather, weight):
    c = P.segment_case(4, perm=perm, gather=gather, weight=weight)
    m, n = c["M"], c["N"]
    assert (c["perm"] is not None) == perm and (c["send"] is not None) == gather and (c["weight"] is not None) == weight
    assert np.array_equal(np.sort(c["order"]), np.arange(m))
    srt = c["recv"][c["order"]]
    assert np.all(np.diff(srt) >= 0) and np.array_equal(np.bincount(srt, minlength=n), P.SEGMENT_LENGTHS)
    if perm:
        assert np.array_equal(c["order"], np.argsort(c["recv"], kind="stable")) and np.any(np.diff(c["recv"]) < 0)
    if gather:
        assert c["x"].shape == (P.GATHER_ROWS, 4)
        assert np.sum(c["send"] < 0) == 3 and np.sum(c["send"] >= P.GATHER_ROWS) == 3
    if weight:
        lo, hi = c["ptr"][P.ZERO_WEIGHT_SEGMENT], c["ptr"][P.ZERO_WEIGHT_SEGMENT + 1]
        w = c["weight"][c["order"]][lo:hi]
        s = np.float32(0)
        for v in w:
            s = np.float32(s + v)
        assert s == 0 and np.all(w != 0)
        assert np.all(P.segment_reference(c, P.SUM, np.float32, normalize=True)[P.ZERO_WEIGHT_SEGMENT] == 0)
        assert np.any(P.segment_reference(c, P.SUM, np.float32)[P.ZERO_WEIGHT_SEGMENT] != 0)


@pytest.mark.parametrize("perm", [False, True])
def test_signed_data_puts_the_extreme_in_the_last_row(perm):
    for kind, op, sign in (("negative", P.MAX, -1), ("positive", P.MIN, 1)):
        c = P.segment_case(3, perm=perm, data=kind)
        rows = c["x"][c["order"]]
        assert np.all(sign * rows > 0)
        ref = P.segment_reference(c, op, np.float32)
        for s, n in enumerate(P.SEGMENT_LENGTHS):
            if n:
                assert np.all(rows[c["ptr"][s + 1] - 1] == sign * 0.5) and np.all(ref[s] == sign * 0.5)
                if n > 1:
                    assert np.all(sign * rows[c["ptr"][s]:c["ptr"][s + 1] - 1] >= 1.0)
            else:
                assert np.all(ref[s] == 0)


def test_fold_is_the_sequential_float32_sum():
    c = P.segment_case(3)
    ref = P.fold_segments(c["x"], c["ptr"], P.SUM, np.float32)
    for s in (1, 8, 15, 16):
        acc = np.zeros(3, np.float32)
        for e in range(c["ptr"][s], c["ptr"][s + 1]):
            acc = (acc + c["x"][e]) if e > c["ptr"][s] else c["x"][e].copy()
        assert np.array_equal(acc, ref[s])
    assert np.array_equal(P.fold_segments(c["x"], c["ptr"], P.MAX, np.float32)[16], c["x"][c["ptr"][16]:c["ptr"][17]].max(0))


@pytest.mark.parametrize("width", P.SEGMENT_WIDTHS)
def test_segment_restatements_within_half_cap(width):
    for perm in (False, True):
        for gather in (False, True):
            plain = P.segment_case(width, perm=perm, gather=gather, data="grid")
            _half("segment mean perm %d gather %d F=%d" % (perm, gather, width),
                  P.segment_reference(plain, P.MEAN, np.float32), P.segment_reference(plain, P.MEAN, np.float64), MEAN_RTOL)
            c = P.segment_case(width, perm=perm, gather=gather, weight=True, data="grid")
            for op, norm in ((P.SUM, False), (P.SUM, True), (P.MEAN, False), (P.MAX, False), (P.MIN, True)):
                _half("weighted op %d normalize %d perm %d gather %d F=%d" % (op, norm, perm, gather, width),
                      P.segment_reference(c, op, np.float32, norm), P.segment_reference(c, op, np.float64, norm),
                      WEIGHTED_RTOL)
    for perm in (False, True):
        g = P.segment_case(width, perm=perm, gather=True)
        for code in P.ACT_NAMES:
            _half("gather-reduce act %d perm %d F=%d" % (code, perm, width),
                  P.segment_reference(g, P.SUM, np.float32, act_code=code),
                  P.segment_reference(g, P.SUM, np.float64, act_code=code))


def test_pool_graph_cases():
    assert P.POOL_GRAPH_ROWS == (0, 1, 16, 17, 5000, 0)
    c = P.pool_case(4)
    assert c["splits"].dtype == np.int64 and c["splits"][-1] == c["x"].shape[0] == 5034
    assert P.POOL_MANY_GRAPHS * (P.POOL_MANY_WIDTH // 4) > P.GRID_CAP
    for width in (3, 4):
        c = P.pool_case(width)
        _half("pool_graph mean F=%d" % width, P.fold_segments(c["grid"], c["splits"], P.MEAN, np.float32),
              P.fold_segments(c["grid"], c["splits"], P.MEAN, np.float64), MEAN_RTOL)
        w32 = c["grid"] * c["weight"][:, None]
        w64 = c["grid"].astype(np.float64) * c["weight"].astype(np.float64)[:, None]
        _half("pool_graph weighted sum F=%d" % width, P.fold_segments(w32, c["splits"], P.SUM, np.float32),
              P.fold_segments(w64, c["splits"], P.SUM, np.float64), WEIGHTED_RTOL)


@pytest.mark.parametrize("perm", [False, True])
def test_segment_softmax_case(perm):
    c = P.softmax_case(perm)
    rows = c["x"][c["order"]]
    lo, hi = c["ptr"][c["equal_segment"]], c["ptr"][c["equal_segment"] + 1]
    assert np.all(np.delete(rows[:, 0], np.arange(lo, hi)) > 9990) and np.abs(rows[:, 1:]).max() < 10
    assert hi - lo == 16 and np.all(rows[lo:hi] == np.float32(0.7))
    r32, r64 = P.segment_softmax_reference(c, np.float32), P.segment_softmax_reference(c, np.float64)
    assert np.allclose(r64[c["order"]][lo:hi], 1 / 16)
    ids = c["recv"].astype(np.int64)
    assert np.allclose(ko.segment_softmax(rows.astype(np.float64), np.sort(ids)), r64[c["order"]], rtol=1e-12)
    sums = np.zeros((c["N"], 3))
    np.add.at(sums, ids, r64)
    assert np.allclose(sums[np.asarray(P.SEGMENT_LENGTHS) > 0], 1.0)
    _half("segment softmax perm %d" % perm, r32, r64)


def test_relational_case():
    c = P.relational_case()
    keep = (c["rel"] >= 0) & (c["rel"] < c["R"])
    assert np.sum(c["rel"] < 0) > 10 and np.sum(c["rel"] >= c["R"]) > 10
    assert np.sum((c["recv"] == 5) & (c["rel"] == 1)) >= P.RELATIONAL_HUB
    assert np.any(np.signbit(c["val"]) & (c["val"] == 0)) and np.any(c["val"] > 0) and np.any(c["val"] < 0)
    negzero = np.signbit(c["val"][:, 0]) & (c["val"][:, 0] == 0) & keep
    assert any(np.any(c["val"][keep & (c["recv"] == a) & (c["rel"] == b), 0] < 0)            # a -0.0 update of a slot whose
               for a, b in zip(c["recv"][negzero], c["rel"][negzero]))                      # minimum is below 0
    ind = np.stack([c["recv"][keep], c["rel"][keep]], 1).astype(np.int64)
    zero = np.zeros((c["N"], c["R"], 4), np.float32)
    mx = ko.tensor_scatter_nd_ops_by_name("max", zero, ind, c["val"][keep])
    mn = ko.tensor_scatter_nd_ops_by_name("min", zero, ind, c["val"][keep])
    assert np.all(mx[2, 0] == 0) and np.all(mn[3, 2] == 0)          # the zero start wins over a one-signed slot
    assert np.all(mx[c["N"] - 1] == 0) and np.all(mn[c["N"] - 1] == 0)
    s32 = ko.tensor_scatter_nd_ops_by_name("sum", zero, ind, c["val"][keep])
    s64 = ko.tensor_scatter_nd_ops_by_name("sum", zero.astype(np.float64), ind, c["val"][keep].astype(np.float64))
    _half("relational scatter sum", s32, s64)


# ---------------------------------------------------------------------------------------------- B. gathers, index
def test_gather_totals_straddle_the_grid_cap():
    assert P.GRID_CAP == 524288 and P.GATHER_TOTALS == (524287, 524288, 524289, 4 * 524288 + 37)
    for total in P.GATHER_TOTALS:
        c4 = P.gather_case(total, 1, 4, [0], k=1)
        c1 = P.gather_case(total, 1, 1, [0], k=1)
        assert P.gather_items(c4, vector=True) == total and P.gather_items(c1, vector=False) == total
        assert np.sum(c4["cols"] == -1) >= 1 and np.sum(c4["cols"] == P.GATHER_TABLE) >= 1
    assert P.gather_items(P.gather_case(P.GRID_CAP // 4, 1, 4, [0], k=1), vector=False) == P.GRID_CAP   # misaligned view
    c = P.gather_case(65537, 2, 16, [1, 0], k=2)
    assert P.gather_items(c, vector=True) > P.GRID_CAP
    ref = P.gather_reference(P.gather_case(50, 3, 3, [3, 0, 2]))
    c = P.gather_case(50, 3, 3, [3, 0, 2])
    assert ref.shape == (50, 3, 3)
    e = int(np.nonzero(c["cols"][0] == -1)[0][0])
    assert not ref[e].any()
    e = int(np.nonzero((c["cols"][3] >= 0) & (c["cols"][3] < P.GATHER_TABLE))[0][0])
    assert np.array_equal(ref[e, 0], c["x"][c["cols"][3, e]]) and np.array_equal(ref[e, 2], c["x"][c["cols"][2, e]])


@pytest.mark.parametrize("g,m", P.INDEX_CASES)
def test_index_batches(g, m):
    assert P.PREP_LDS_GRAPHS == 1023 and P.INDEX_LONG == P.GRID_CAP + 67
    assert {c[0] for c in P.INDEX_CASES} == {1, 1023, 1024, 1025} and {c[1] for c in P.INDEX_CASES} == {1, 63, 64, 65, P.INDEX_LONG}
    b = P.index_batch(g, m)
    ns, es = b["node_splits"], b["edge_splits"]
    assert len(ns) == len(es) == g + 1 and es[-1] == m and b["idx"].shape == (m, 2) and b["idx"].dtype == np.int64
    if g >= 3:
        for q in (0, g // 2, g - 1):
            assert ns[q + 1] == ns[q] and es[q + 1] == es[q]
    n_of = np.diff(ns)[b["graph"]]
    assert np.all(b["idx"] >= 0) and np.all(b["idx"] < n_of[:, None])
    cols, flags = P.index_reference(b)
    assert flags == 0 and cols.shape == (2, m) and cols.dtype == np.int32
    assert np.array_equal(cols.T, b["idx"] + ns[b["graph"]][:, None])
    if g >= 1023 and m >= 63:
        assert P.local_descents_across_graphs(b, 0) > 0 and P.local_descents_across_graphs(b, 1) > 0
    for col, bit in ((0, P.FLAG_UNSORTED_COL0), (1, P.FLAG_UNSORTED_COL1)):
        d = P.with_descent(b, col)
        assert m > 1 or d is None
        if d is not None:
            assert P.index_reference(d)[1] == bit
        o = P.with_oob(b, col)
        oc, of = P.index_reference(o)
        assert of == P.FLAG_OOB
        gl = b["graph"][-1]
        assert oc[col, -1] == ns[gl + 1] - 1 and o["idx"][-1, col] == ns[gl + 1] - ns[gl]
    if m > P.GRID_CAP:
        d = P.with_descent(b, 0)
        assert int(np.nonzero(d["idx"][:, 0] != b["idx"][:, 0])[0][0]) >= P.GRID_CAP      # found on the second trip
    for k in (1, 3):
        bk = P.index_batch(g, m, k=k)
        ck, fk = P.index_reference(bk)
        assert fk == 0 and ck.shape == (k, m)


def test_descent_cases_exist_where_the_gpu_test_needs_them():
    for g in (1, 1023, 1024, 1025):
        for m in (63, 64, 65):
            assert P.with_descent(P.index_batch(g, m), 0) is not None, (g, m)


def test_csr_and_sort_cases():
    cases = P.csr_cases()
    seg, n = cases["gaps"]
    ptr = P.csr_reference(seg, n)
    assert ptr[0] == 0 and ptr[-1] == len(seg) and np.any(np.diff(ptr) == 0) and np.all(np.diff(ptr) >= 0)
    assert np.array_equal(np.diff(ptr), np.bincount(seg, minlength=n))
    seg, n = cases["one-segment"]
    assert np.array_equal(np.diff(P.csr_reference(seg, n)), [0, 0, 0, 0, 700, 0, 0, 0, 0])
    seg, n = cases["empty"]
    assert not P.csr_reference(seg, n).any()
    seg, n = cases["above-n"]
    assert seg.max() > n and P.csr_reference(seg, n)[-1] == len(seg) - 3
    seg, n = cases["second-trip"]
    assert len(seg) + 1 > P.GRID_CAP
    keys = P.sort_cases()
    assert len(keys["one"]) == 1 and len(keys["few-keys"]) == 70000 and len(np.unique(keys["few-keys"])) == 5


# --------------------------------------------------------------------------------------------------- C. Dense
def test_dense_triples_cover_every_size():
    t = P.dense_triples()
    assert len(t) == len(set(t)) == 40
    for axis, values in enumerate((P.DENSE_R, P.DENSE_K, P.DENSE_U)):
        for v in values:
            assert sum(1 for s in t if s[axis] == v) >= 2, (axis, v)
    assert sum(P.vec_eligible(k, u) for _, k, u in t) >= 4 and sum(not P.vec_eligible(k, u) for _, k, u in t) >= 20
    assert any(k < 4 for _, k, _ in t) and any(u < 4 for _, _, u in t)
    assert any(k % 2 == 1 and k > 64 for _, k, _ in t)               # an odd K whose last k pair is zero padded
    assert any(P.vec_eligible(k, u) and r > 64 and k > 64 for r, k, u in t)


@pytest.mark.parametrize("bias", [True, False])
def test_dense_restatements_within_half_cap(bias):
    worst = 0.0
    for r, k, u in P.dense_triples():
        c = P.dense_case(r, k, u)
        worst = max(worst, _half("dense %s bias %d" % ((r, k, u), bias), P.dense_reference(c, np.float32, bias)[0],
                                 P.dense_reference(c, np.float64, bias)[0]))
    print("[restatement] dense worst of 40 triples, bias %d: %.2e" % (bias, worst))


@pytest.mark.parametrize("shape", P.DENSE_EX_SHAPES)
def test_dense_ex_restatements_within_half_cap(shape):
    c = P.dense_case(*shape)
    for code in P.ACT_NAMES:
        for kw in ({"in_mode": 1, "in_act": code}, {"in_mode": 2, "in_act": code},
                   {"act_code": 2, "in_act": code, "grad_pre": True}):
            _half("dense_ex %s %s" % (shape, kw), P.dense_reference(c, np.float32, **kw)[0],
                  P.dense_reference(c, np.float64, **kw)[0])
    for kw in ({"act_code": 4}, {"act_code": 2, "addend": True}):
        a, b = P.dense_reference(c, np.float32, **kw), P.dense_reference(c, np.float64, **kw)
        _half("dense_ex %s %s out" % (shape, kw), a[0], b[0])
        _half("dense_ex %s %s pre" % (shape, kw), a[1], b[1])


def test_splitk_cases():
    assert P.SPLITK_CASES == ((64, 4), (100, 64), (1433, 3), (1433, 11), (512, 64))
    used = {ks: P.splitk_used(*ks) for ks in P.SPLITK_CASES}
    assert used == {(64, 4): 1, (100, 64): 2, (1433, 3): 3, (1433, 11): 8, (512, 64): 8}
    assert used[(64, 4)] < 4 and used[(100, 64)] < 64                 # trailing empty slices are dropped
    assert P.layer_takes_splitk(100, 512, 64) and not P.layer_takes_splitk(100, 511, 64)
    assert P.layer_takes_splitk(64 * 128, 512, 64) and not P.layer_takes_splitk(64 * 128 + 1, 512, 64)
    for k, _ in P.SPLITK_CASES:
        c = P.dense_case(P.SPLITK_R, k, P.SPLITK_U)
        _half("split-K K=%d" % k, P.dense_reference(c, np.float32)[0], P.dense_reference(c, np.float64)[0])


@pytest.mark.parametrize("c", P.ROW_WIDTHS)
def test_row_kernels_restatements(c):
    assert P.ROW_WIDTHS == (1, 7, 63, 64, 65, 129, 1000) and P.ROWS_SECOND_TRIP * 64 > P.GRID_CAP
    case = P.rows_case(c)
    assert np.all(case["x"][0] > 9990) and np.all(case["x"][1] == case["x"][1, 0])
    y32, y64 = P.softmax_rows(case["x"], np.float32), P.softmax_rows(case["x"], np.float64)
    assert np.allclose(y64.sum(1), 1) and np.allclose(y64[1], 1 / c)
    _half("softmax rows C=%d" % c, y32, y64)
    _half("softmax rows grad C=%d" % c, P.softmax_rows_grad(y32, case["g"], np.float32),
          P.softmax_rows_grad(y32, case["g"], np.float64))
    for gamma, beta in ((case["gamma"], case["beta"]), (None, case["beta"]), (case["gamma"], None), (None, None)):
        # row 0 (entries near 1e4 with unit spread) is left to the softmax: x - mean loses 1e4 / spread ~ 13 bits there
        r32, r64 = (P.layer_norm(case["x"][1:], gamma, beta, 1e-3, t) for t in (np.float32, np.float64))
        if beta is not None:
            assert np.allclose(r64[0], beta)                           # the constant row: (x - mean) = 0
        _half("layer norm C=%d gamma %d beta %d" % (c, gamma is not None, beta is not None), r32, r64)


# ------------------------------------------------------------------------------------------- D. parameter gradients
def test_wgrad_shapes_cover_the_chunk_plan():
    shapes = P.wgrad_shapes()
    assert len(shapes) == len(set(shapes)) == 21
    for r in P.WGRAD_R:
        assert sum(1 for s in shapes if s[0] == r) >= 2
    for ku in P.WGRAD_KU:
        assert sum(1 for s in shapes if s[1:] == ku) >= 2, ku
    plans = {s: P.wgrad_plan(*s) for s in shapes}
    for (r, k, u), (rows, chunks) in plans.items():
        assert rows % 32 == 0 and (chunks - 1) * rows < r <= chunks * rows
    chunks = [c for _, c in plans.values()]
    assert 1 in chunks                                                            # one chunk: no workspace, no reduce
    assert any(c >= 8 and c % 8 == 0 for c in chunks)                             # the reduce kernel's 8-at-a-time body alone
    assert any(c > 8 and c % 8 != 0 for c in chunks)                              # body and remainder
    assert any(1 < c < 8 for c in chunks)                                         # remainder alone
    assert any(c > 1 and r - (c - 1) * rows < 32 for (r, _, _), (rows, c) in plans.items())     # a short last chunk
    assert any(rows > 32 and c > 1 for rows, c in plans.values())                 # more than one LDS stage per chunk
    assert any(k % 4 == 0 and u % 4 == 0 for _, k, u in shapes) and any(k % 4 or u % 4 for _, k, u in shapes)
    for s, p in sorted(plans.items()):
        print("[plan] wgrad R=%d K=%d U=%d: %d rows per chunk, %d chunks" % (s + p))


def test_wgrad_restatements_within_half_cap():
    for s in P.wgrad_shapes():
        c = P.wgrad_case(*s)
        (w32, b32), (w64, b64) = P.wgrad_reference(c, np.float32), P.wgrad_reference(c, np.float64)
        _half("wgrad dW %s" % (s,), w32, w64)
        _half("wgrad db %s" % (s,), b32[None], b64[None])              # the bias gradient is one row


def test_embedding_grad_cases():
    assert {s[0] for s in P.EMBED_GRAD_SHAPES} == {1, 5000} and {s[1] for s in P.EMBED_GRAD_SHAPES} == {1, 95}
    assert {s[2] for s in P.EMBED_GRAD_SHAPES} == {1, 64, 130}
    for n, vocab, dim in P.EMBED_GRAD_SHAPES:
        c = P.embedding_grad_case(n, vocab, dim)
        ids = P.embedding_ids(c["numbers"], vocab)
        assert c["numbers"].shape == (n,) and c["g"].shape == (n, dim)
        ref = P.embedding_grad_reference(c, vocab, np.float32)
        assert ref.shape == (vocab, dim)
        if n == 5000:
            assert np.sum(ids == c["hub"]) == P.EMBED_HUB_ROWS and np.sum(ids == vocab) > 10
            assert np.any(c["numbers"] < 0) and np.any(c["numbers"] >= vocab) and np.any(c["numbers"] % 1 != 0)
            acc = np.zeros(dim, np.float32)
            for i in np.nonzero(ids == c["hub"])[0]:
                acc = acc + c["g"][i]
            assert np.array_equal(acc, ref[c["hub"]])
        else:
            assert np.array_equal(ref[ids[0]], c["g"][0]) and np.count_nonzero(ref.any(axis=1)) == 1


# ----------------------------------------------------------------------------------------------------- E. GCN tiles
def _gcn_oracle(case, dtype):
    return ko.gcn_forward(ko.to_dtype(case["params"], dtype), ko.R(case["attrs"].astype(dtype), case["ns"]),
                          ko.R(case["w"].astype(dtype), case["es"]), ko.R(case["idx"], case["es"]), depth=2,
                          output_mlp_act=("relu", "linear")).values


@pytest.mark.parametrize("units,hub", P.GCN_HUB_CASES)
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_gcn_hub_cases(units, hub, order):
    assert P.GCN_ECAP == {128: 768, 64: 1792, 32: 1792}
    deg = P.gcn_degrees(40, seed=hub, hub=hub)
    assert deg[P.GCN_HUB_NODE] == hub and np.all(np.delete(deg, P.GCN_HUB_NODE) <= 6) and 0 in deg
    starts = P.gcn_tiles(deg)
    assert starts is not None and np.any(np.diff(starts) < 16) and np.all(np.diff(starts) >= 1)
    assert P.GCN_HUB_NODE in starts and P.GCN_HUB_NODE + 1 in starts            # the hub is a tile of its own
    assert P.gcn_windows(deg, units) == {769: 2, 1793: 2, 3600: 3}[hub]
    if hub in (769, 1793):
        assert hub - P.GCN_ECAP[units] == 1                                      # the second window holds one edge
    c = P.gcn_case(deg, 20, units, order=order)
    assert np.array_equal(np.bincount(c["idx"][:, 0], minlength=40), deg)
    assert np.all(np.diff(c["idx"][:, 0]) >= 0) == (order == "sorted")
    assert c["w"].min() >= 0.05 and c["w"].max() <= 1.0
    _half("GCN hub %d edges, %d units, %s" % (hub, units, order), _gcn_oracle(c, np.float32), _gcn_oracle(c, np.float64))


def test_gcn_boundary_cases():
    d512, d513 = P.gcn_uniform_degrees(512), P.gcn_uniform_degrees(513)
    assert d512[:16].sum() == 512 and d513[:16].sum() == 513 and d512[16:].max() <= 6
    assert P.gcn_tiles(d512) is None
    starts = P.gcn_tiles(d513)
    assert starts is not None and np.any(np.diff(starts) < 16)
    for name, deg, feats in (("uniform tile of 512 edges", d512, 20), ("uniform tile of 513 edges", d513, 20),
                             ("17 nodes", P.gcn_degrees(17, 1), 20), ("33 nodes", P.gcn_degrees(33, 2), 20),
                             ("528 features", P.gcn_degrees(20, 3), 528), ("529 features", P.gcn_degrees(20, 3), 529)):
        assert P.gcn_tiles(deg) is None or name.endswith("513 edges")
        c = P.gcn_case(deg, feats, 64)
        _half("GCN %s" % name, _gcn_oracle(c, np.float32), _gcn_oracle(c, np.float64))
    assert 17 % 16 == 1 and 33 % 16 == 1
    # input launch: 16-k blocks dealt to four waves, eight steps per trip of the pipeline loop
    for feats, ragged in ((528, False), (529, True)):
        full = feats // 16
        assert full == 33 and (feats % 16 != 0) == ragged
        assert max((full - w + 3) // 4 for w in range(4)) == 9                   # wave 0 owns nine blocks: a second trip
