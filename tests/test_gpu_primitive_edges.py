"""The layer-path kernels off the tiny random graphs (tests/primitive_cases.py): segment reductions with 16- and 8-row
rounds, all eight perm / gather / weight instantiations and the scalar build; gathers, index preparation and elementwise
kernels above the 524 288-thread grid cap; index preparation around 1023 graphs; the Dense family at k / row / column
tails, its prologue and epilogue forms and split-K; the weight gradient across its chunk plan; the GCN tile kernel with
more than one edge window, a tile table and a second trip of its input pipeline.

Index, gather, max / min and unweighted-sum results are compared for equality.  Floating-point results go through
``parity.assert_rows_close`` with its default caps; the only other figures are the two tests/test_gpu_layers.py states for
the same kernel: 1e-6 for ``mean`` (test_pooling_local_edges) and 2e-6 for weighted pooling
(test_pooling_weighted_local_edges).  Cases held to those two figures use operands on a binary grid, whose float32 sums
are exact.

Distance of the float32 restatement from its float64 twin (rowwise_rel; asserted below half the cap by
tests/test_primitive_cases.py, which prints each figure):

  A  segment mean; weighted sum / mean / max / min, plain and normalised (grid operands)   <= 5.7e-08 (half caps 5e-07, 1e-06)
     gather-reduce + activation, 10 codes x 5 widths, normal deviates, 1000-row segment     7.0e-08 .. 5.8e-06
     pool_graph mean / weighted sum, 5000-row graph (grid operands)                         <= 4.1e-08
     segment softmax, one column near 1e4, without / with perm                              6.6e-07 / 1.3e-06
     relational scatter sum, hub slot of 1000 edges                                         4.7e-07
  C  dense, 40 (R, K, U) triples                                  <= 6.3e-07 with bias, <= 6.2e-07 without
     dense_ex prologue 1 / 2, grad_pre, out_pre, addend           (65, 66, 68) <= 6.8e-07, (65, 128, 384) <= 8.0e-07
     split-K operands, K = 64 100 512 1433                        4.2e-07 .. 7.9e-07
     softmax rows <= 1.9e-07, its reverse <= 1.4e-07, layer norm <= 1.6e-07   (C = 1 .. 1000)
  D  dense wgrad, 21 shapes                                       dW <= 1.8e-06, db (one row) <= 4.7e-06
  E  GCN hub of 769 / 1793 / 3600 edges, sorted and shuffled      5.2e-07 .. 2.9e-06
     GCN 512 / 513 edges in the busiest uniform tile              6.8e-07 / 4.9e-07
     GCN 17 / 33 nodes 3.5e-07 / 4.5e-07; 528 / 529 input features 7.8e-07 / 4.2e-06
"""
import ctypes

import numpy as np
import pytest
import torch

import primitive_cases as P
from gcnn_keras_amd import _ffi
from gcnn_keras_amd.ragged import RaggedTensor
from oracle import kgcnn_oracle as ko
from parity import BAR_CAP, RTOL, assert_rows_close, rowwise_rel

pytestmark = pytest.mark.gpu

MEAN_RTOL = 1e-6        # tests/test_gpu_layers.py::test_pooling_local_edges holds ``mean`` to this
WEIGHTED_RTOL = 2e-6    # tests/test_gpu_layers.py::test_pooling_weighted_local_edges


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _misaligned(t):
    """The same values at an address 4 bytes past a 16-byte boundary (a view of ``buf[1:]``)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _bits(got, ref, what=""):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float32, (what, got.shape, ref.shape)
    bad = np.nonzero(got.view(np.uint32) != ref.view(np.uint32))
    assert bad[0].size == 0, "%s: %d elements differ, first at %s: %r vs %r" % (
        what, bad[0].size, tuple(int(b[0]) for b in bad), got[tuple(b[0] for b in bad)], ref[tuple(b[0] for b in bad)])


def _exact(got, ref, what=""):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    assert np.array_equal(got, ref), "%s: %d elements differ" % (what, int(np.sum(got != ref)))


def _out(*shape):
    """An output buffer filled with NaN: an element the kernel does not write fails every comparison."""
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


# ======================================================================================== A. segment reductions
def _reduce(case, op, normalize=False, act=0, misalign=False):
    x = _t(case["x"])
    if misalign:
        x = _misaligned(x)
    ptr, perm, w, send = _t(case["ptr"]), _t(case["perm"]), _t(case["weight"]), _t(case["send"])
    n, f = case["N"], case["width"]
    out = _out(n, f)
    if send is None:
        assert act == 0
        _ffi.call("mp_segment_reduce_csr_f32", op, _ffi.ptr(x), case["M"], f, _ffi.ptr(ptr), _ffi.ptr(perm), n,
                  _ffi.ptr(w), int(normalize), _ffi.ptr(out), _ffi.stream())
    else:
        _ffi.call("mp_gather_segment_reduce_csr_f32", op, _ffi.ptr(x), P.GATHER_ROWS, f, _ffi.ptr(send), case["M"],
                  _ffi.ptr(ptr), _ffi.ptr(perm), n, _ffi.ptr(w), int(normalize), act, P.ALPHA, _ffi.ptr(out),
                  _ffi.stream())
    return _np(out)


_EMPTY = [i for i, n in enumerate(P.SEGMENT_LENGTHS) if n == 0]


@pytest.mark.parametrize("width", P.SEGMENT_WIDTHS)
@pytest.mark.parametrize("perm", [False, True])
@pytest.mark.parametrize("gather", [False, True])
def test_segment_sum_max_min_equal_the_sequential_fold(width, perm, gather):
    """The four unweighted instantiations: sum equals the float32 fold in edge order bit for bit, max and min equal NumPy,
    rows without edges are exactly 0; mean (grid operands) is held to the 1e-6 of test_pooling_local_edges."""
    case = P.segment_case(width, perm=perm, gather=gather)
    for op, name in ((P.SUM, "sum"), (P.MAX, "max"), (P.MIN, "min")):
        got = _reduce(case, op)
        _bits(got, P.segment_reference(case, op, np.float32), "%s F=%d perm %d gather %d" % (name, width, perm, gather))
        assert not got[_EMPTY].any() and not np.signbit(got[_EMPTY]).any()
        if op != P.SUM:
            rows = P.segment_rows(case, np.float32)
            for s in (5, 13, 15, 16):
                part = rows[case["ptr"][s]:case["ptr"][s + 1]]
                _exact(got[s], part.max(axis=0) if op == P.MAX else part.min(axis=0), "%s of segment %d" % (name, s))
    grid = P.segment_case(width, perm=perm, gather=gather, data="grid")
    assert_rows_close(_reduce(grid, P.MEAN), P.segment_reference(grid, P.MEAN, np.float32),
                      P.segment_reference(grid, P.MEAN, np.float64), rtol=MEAN_RTOL, what="segment mean F=%d" % width)


@pytest.mark.parametrize("width", [1, 4, 130])
@pytest.mark.parametrize("perm", [False, True])
def test_segment_extreme_in_the_last_slot_of_the_last_round(width, perm):
    """All-negative rows whose maximum sits in the segment's last row (and the mirror image for min): a masked tail slot
    that leaks, a dropped last row or an accumulator that starts at 0 changes the result."""
    for kind, op, value in (("negative", P.MAX, -0.5), ("positive", P.MIN, 0.5)):
        case = P.segment_case(width, perm=perm, data=kind)
        got = _reduce(case, op)
        _bits(got, P.segment_reference(case, op, np.float32), kind)
        live = np.asarray(P.SEGMENT_LENGTHS) > 0
        assert np.all(got[live] == np.float32(value)) and not got[~live].any()
        _bits(_reduce(case, P.SUM), P.segment_reference(case, P.SUM, np.float32), kind + " sum")


@pytest.mark.parametrize("width", P.SEGMENT_WIDTHS)
@pytest.mark.parametrize("perm", [False, True])
@pytest.mark.parametrize("gather", [False, True])
def test_segment_weighted(width, perm, gather):
    """The four weighted instantiations, plain and normalised by the weight sum, held to the 2e-6 of
    test_pooling_weighted_local_edges; the segment whose weights sum to 0 gives 0 under normalisation."""
    case = P.segment_case(width, perm=perm, gather=gather, weight=True, data="grid")
    for op, norm in ((P.SUM, False), (P.SUM, True), (P.MEAN, False), (P.MAX, False), (P.MIN, True)):
        got = _reduce(case, op, normalize=norm)
        assert_rows_close(got, P.segment_reference(case, op, np.float32, norm), P.segment_reference(case, op, np.float64, norm),
                          rtol=WEIGHTED_RTOL, what="weighted op %d normalize %d F=%d" % (op, norm, width))
        assert not got[_EMPTY].any()
        if norm:
            assert not got[P.ZERO_WEIGHT_SEGMENT].any()
        elif op == P.SUM:
            assert got[P.ZERO_WEIGHT_SEGMENT].any()


@pytest.mark.parametrize("code", sorted(set(_ffi.ACTIVATION_CODES.values())))
def test_gather_reduce_activation(code):
    assert code in P.ACT_NAMES and _ffi.ACTIVATION_CODES[P.ACT_NAMES[code]] == code
    for width, perm in ((4, True), (3, False), (130, True)):
        case = P.segment_case(width, perm=perm, gather=True)
        got = _reduce(case, P.SUM, act=code)
        assert_rows_close(got, P.segment_reference(case, P.SUM, np.float32, act_code=code),
                          P.segment_reference(case, P.SUM, np.float64, act_code=code),
                          what="gather-reduce act %d F=%d" % (code, width))
        assert np.max(np.abs(got[_EMPTY] - P.act(code, np.zeros(1, np.float32)))) <= 1e-7        # act(0) in the empty rows


@pytest.mark.parametrize("width", [4, 128])
@pytest.mark.parametrize("perm", [False, True])
@pytest.mark.parametrize("gather", [False, True])
def test_segment_scalar_build_gives_the_vector_build_bits(width, perm, gather):
    """A 4-byte-offset operand takes the one-float build: same rows, same order, same bits."""
    case = P.segment_case(width, perm=perm, gather=gather)
    for op in (P.SUM, P.MAX, P.MEAN):
        _bits(_reduce(case, op, misalign=True), _reduce(case, op), "op %d F=%d" % (op, width))
    _bits(_reduce(case, P.SUM, misalign=True), P.segment_reference(case, P.SUM, np.float32), "scalar build sum")


def _pool(op, x, splits, weight=None, misalign=False):
    xd = _misaligned(_t(x)) if misalign else _t(x)
    g = len(splits) - 1
    out = _out(g, x.shape[1])
    sd, wd = _t(splits), _t(weight)
    _ffi.call("mp_pool_graph_f32", op, _ffi.ptr(xd), _ffi.ptr(sd), g, x.shape[1], _ffi.ptr(wd), _ffi.ptr(out), _ffi.stream())
    return _np(out)


@pytest.mark.parametrize("width", [3, 4, 128])
def test_pool_graph_int64_splits(width):
    case = P.pool_case(width)
    x, splits = case["x"], case["splits"]
    for op in (P.SUM, P.MAX, P.MIN):
        got = _pool(op, x, splits)
        _bits(got, P.fold_segments(x, splits, op, np.float32), "pool_graph op %d F=%d" % (op, width))
        assert not got[[0, -1]].any()
    if width % 4 == 0:
        _bits(_pool(P.SUM, x, splits, misalign=True), _pool(P.SUM, x, splits), "pool_graph scalar build")
    grid = case["grid"]
    assert_rows_close(_pool(P.MEAN, grid, splits), P.fold_segments(grid, splits, P.MEAN, np.float32),
                      P.fold_segments(grid, splits, P.MEAN, np.float64), rtol=MEAN_RTOL, what="pool_graph mean")
    w32 = grid * case["weight"][:, None]
    w64 = grid.astype(np.float64) * case["weight"].astype(np.float64)[:, None]
    assert_rows_close(_pool(P.SUM, grid, splits, case["weight"]), P.fold_segments(w32, splits, P.SUM, np.float32),
                      P.fold_segments(w64, splits, P.SUM, np.float64), rtol=WEIGHTED_RTOL, what="pool_graph weighted")


def test_pool_graph_second_grid_stride_trip():
    g, f = P.POOL_MANY_GRAPHS, P.POOL_MANY_WIDTH
    assert g * (f // 4) > P.GRID_CAP
    x = np.random.default_rng(3).normal(size=(g, f)).astype(np.float32)
    splits = np.arange(g + 1, dtype=np.int64)
    for op in (P.SUM, P.MAX, P.MEAN):
        _bits(_pool(op, x, splits), x, "one row per graph, op %d" % op)


@pytest.mark.parametrize("perm", [False, True])
def test_segment_softmax(perm):
    case = P.softmax_case(perm)
    a, ptr, pm = _t(case["x"]), _t(case["ptr"]), _t(case["perm"])
    out = _out(case["M"], case["width"])
    _ffi.call("mp_segment_softmax_csr_f32", _ffi.ptr(a), case["M"], case["width"], _ffi.ptr(ptr), _ffi.ptr(pm), case["N"],
              _ffi.ptr(out), _ffi.stream())
    got = _np(out)
    order = case["order"]
    ids = np.sort(case["recv"].astype(np.int64))
    ref32, ref64 = np.empty_like(got), np.empty(got.shape, np.float64)
    ref32[order] = ko.segment_softmax(case["x"][order], ids)
    ref64[order] = ko.segment_softmax(case["x"][order].astype(np.float64), ids)
    assert_rows_close(got, ref32, ref64, what="segment softmax")
    assert_rows_close(got, P.segment_softmax_reference(case, np.float32), ref64, what="segment softmax (restatement)")
    sums = np.zeros((case["N"], case["width"]))
    np.add.at(sums, case["recv"].astype(np.int64), got.astype(np.float64))
    live = np.asarray(P.SEGMENT_LENGTHS) > 0
    assert np.max(np.abs(sums[live] - 1.0)) <= RTOL and not sums[~live].any()
    lo, hi = case["ptr"][case["equal_segment"]], case["ptr"][case["equal_segment"] + 1]
    assert np.all(got[order][lo:hi] == np.float32(1 / 16))


@pytest.mark.parametrize("op,name", [(P.SUM, "sum"), (P.MAX, "max"), (P.MIN, "min")])
@pytest.mark.parametrize("width", [1, 4])
def test_relational_scatter(op, name, width):
    case = P.relational_case(width)
    val, recv, rel = _t(case["val"]), _t(case["recv"]), _t(case["rel"])
    n, r = case["N"], case["R"]
    out = torch.zeros((n, r, width), dtype=torch.float32, device="cuda")
    _ffi.call("mp_scatter_relational_f32", op, _ffi.ptr(val), len(case["recv"]), width, _ffi.ptr(recv), _ffi.ptr(rel),
              n, r, _ffi.ptr(out), _ffi.stream())
    got = _np(out)
    keep = (case["rel"] >= 0) & (case["rel"] < r)                 # the kernel skips the others
    ind = np.stack([case["recv"][keep], case["rel"][keep]], 1).astype(np.int64)
    zero = np.zeros((n, r, width), np.float32)
    ref32 = ko.tensor_scatter_nd_ops_by_name(name, zero, ind, case["val"][keep])
    if op == P.SUM:
        ref64 = ko.tensor_scatter_nd_ops_by_name(name, zero.astype(np.float64), ind, case["val"][keep].astype(np.float64))
        assert_rows_close(got, ref32, ref64, what="relational scatter sum")
    else:
        _exact(got, ref32, "relational scatter " + name)
        assert not got[2, 0].any() if op == P.MAX else not got[3, 2].any()      # the zero start wins
    assert not got[n - 1].any()


# ==================================================================================== B. gathers and index work
def _gather_rows(case, misalign=False):
    x, cols = _t(case["x"]), _t(case["cols"])
    if misalign:
        x = _misaligned(x)
    out = _out(case["M"], case["ncols"], case["width"])
    _ffi.call("mp_gather_rows_f32", _ffi.ptr(x), P.GATHER_TABLE, case["width"], _ffi.ptr(cols), case["M"], case["ncols"],
              _ffi.int32_array(case["colsel"]), _ffi.ptr(out), _ffi.stream())
    return _np(out)


@pytest.mark.parametrize("total", P.GATHER_TOTALS)
@pytest.mark.parametrize("build", ["float4", "scalar"])
def test_gather_rows_around_the_grid_cap(total, build):
    """Work items one below, at, one above and four times above the grid: the four-chain unroll does work only above it."""
    case = P.gather_case(total, 1, 4 if build == "float4" else 1, [0], k=1)
    assert P.gather_items(case, vector=build == "float4") == total
    _exact(_gather_rows(case), P.gather_reference(case), "gather %d items, %s" % (total, build))


def test_gather_rows_misaligned_view_takes_the_scalar_build():
    case = P.gather_case(P.GRID_CAP // 4 + 3, 1, 4, [0], k=1)
    assert P.gather_items(case, vector=False) > P.GRID_CAP > P.gather_items(case, vector=True)
    _exact(_gather_rows(case, misalign=True), P.gather_reference(case), "misaligned gather")


@pytest.mark.parametrize("colsel", [[2], [1, 0], [3, 0, 2], [3, 2, 1, 0], [1, 1, 1, 1]])
@pytest.mark.parametrize("width", [3, 4, 16])
def test_gather_rows_column_selection(colsel, width):
    m = 65537 if (width == 16 and len(colsel) == 2) else 1000          # 65537 x 2 x 4 chunks: above the grid
    case = P.gather_case(m, len(colsel), width, colsel)
    _exact(_gather_rows(case), P.gather_reference(case), "gather columns %s F=%d" % (colsel, width))


@pytest.mark.parametrize("width", [3, 4])
@pytest.mark.parametrize("col", [-1, 0, 2])
@pytest.mark.parametrize("splits", [True, False])
def test_gather_rows_i64(width, col, splits):
    b = P.index_batch(7, 300, k=3, seed=2)
    idx = b["idx"].copy()
    idx[0, :] = -1                                   # the first edge's graph starts at row 0: -1 stays out of range
    idx[-1, :] = b["N"] + 5
    rng = np.random.default_rng(9)
    x = rng.normal(size=(b["N"], width)).astype(np.float32)
    rows = idx + (b["node_splits"][b["graph"]][:, None] if splits else 0)
    ref = P.take_rows(x, rows if col < 0 else rows[:, col])
    ncols = 3 if col < 0 else 1
    out = _out(b["M"], ncols, width)
    xd, idd, ns, es = _t(x), _t(idx), _t(b["node_splits"]), _t(b["edge_splits"])
    _ffi.call("mp_gather_rows_i64_f32", _ffi.ptr(xd), b["N"], width, _ffi.ptr(idd), b["M"], 3, col,
              _ffi.ptr(ns) if splits else None, _ffi.ptr(es) if splits else None, b["G"], _ffi.ptr(out), _ffi.stream())
    _exact(_np(out).reshape(ref.shape), ref, "gather_rows_i64")


@pytest.mark.parametrize("width", [1, 4, 130])
def test_repeat_rows_with_empty_graphs(width):
    ns, _ = P.batch_splits(9, 10, seed=4)
    g, n = len(ns) - 1, int(ns[-1])
    assert ns[1] == ns[0] and ns[-1] == ns[-2]
    state = np.random.default_rng(width).normal(size=(g, width)).astype(np.float32)
    out = _out(n, width)
    sd, nd = _t(state), _t(ns)
    _ffi.call("mp_repeat_rows_f32", _ffi.ptr(sd), _ffi.ptr(nd), g, width, n, _ffi.ptr(out), _ffi.stream())
    _exact(_np(out), np.repeat(state, np.diff(ns), axis=0), "repeat rows")


@pytest.mark.parametrize("dim", [3, 64])
def test_embedding_truncates_and_flags_numbers_outside_the_table(dim):
    vocab = 95
    table = np.random.default_rng(dim).normal(size=(vocab, dim)).astype(np.float32)

    def run(numbers):
        numbers = np.asarray(numbers, np.float32)
        out, flags = _out(len(numbers), dim), torch.zeros(1, dtype=torch.int32, device="cuda")
        td, nd = _t(table), _t(numbers)
        _ffi.call("mp_embedding_f32", _ffi.ptr(td), vocab, dim, _ffi.ptr(nd), len(numbers), _ffi.ptr(out), _ffi.ptr(flags),
                  _ffi.stream())
        return _np(out), int(flags.item())

    got, flags = run([6.9, 1.0, 94.99, 0.0])
    _exact(got, table[[6, 1, 94, 0]], "in-range numbers")
    assert flags == 0
    for bad in (-1.0, float(vocab)):
        got, flags = run([6.9, bad, 8.0])
        ref = table[[6, 0, 8]].copy()
        ref[1] = 0
        _exact(got, ref, "number %g" % bad)
        assert flags == _ffi.MP_FLAG_OOB


def _prepare(batch):
    idx, ns, es = _t(batch["idx"]), _t(batch["node_splits"]), _t(batch["edge_splits"])
    cols = torch.full((batch["K"], batch["M"]), -7, dtype=torch.int32, device="cuda")
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    _ffi.call("mp_index_prepare_i64", _ffi.ptr(idx), batch["M"], batch["K"], _ffi.ptr(ns), _ffi.ptr(es), batch["G"],
              batch["N"], _ffi.ptr(cols), _ffi.ptr(flags), _ffi.stream())
    return _np(cols), int(flags.item())


def _check_prepare(batch, what):
    cols, flags = _prepare(batch)
    ref_cols, ref_flags = P.index_reference(batch)
    _exact(cols, ref_cols, what)
    assert flags == ref_flags, "%s: flags %d, expected %d" % (what, flags, ref_flags)
    return flags


@pytest.mark.parametrize("g,m", P.INDEX_CASES)
def test_index_prepare_pairs(g, m):
    """K = 2: the LDS search up to 1023 graphs, the wave-uniform search plus walk above; empty graphs first, in the middle
    and last; descents of the sample ids across graph boundaries raise no flag, one inside a graph raises its column's
    flag alone, an id equal to the node count raises MP_FLAG_OOB and is clamped."""
    b = P.index_batch(g, m)
    assert _check_prepare(b, "sorted batch G=%d M=%d" % (g, m)) == 0
    for col, bit in ((0, _ffi.MP_FLAG_UNSORTED_COL0), (1, _ffi.MP_FLAG_UNSORTED_COL1)):
        d = P.with_descent(b, col)
        if d is not None:
            assert _check_prepare(d, "descent in column %d" % col) == bit
        o = P.with_oob(b, col)
        assert _check_prepare(o, "id past the graph in column %d" % col) == _ffi.MP_FLAG_OOB
        assert _prepare(o)[0][col, -1] == b["node_splits"][b["graph"][-1] + 1] - 1


@pytest.mark.parametrize("g,m", [c for c in P.INDEX_CASES if c[1] <= 65] + [(1025, P.INDEX_LONG)])
@pytest.mark.parametrize("k", [1, 3])
def test_index_prepare_other_widths(g, m, k):
    b = P.index_batch(g, m, k=k)
    assert _check_prepare(b, "sorted batch G=%d M=%d K=%d" % (g, m, k)) == 0
    d = P.with_descent(b, 0)
    if d is not None:
        assert _check_prepare(d, "descent in column 0") == _ffi.MP_FLAG_UNSORTED_COL0
    if k == 3:
        d = P.with_descent(b, 2)
        if d is not None:
            assert _check_prepare(d, "descent in the untracked third column") == 0
    o = P.with_oob(b, k - 1)
    assert _check_prepare(o, "id past the graph") == _ffi.MP_FLAG_OOB


@pytest.mark.parametrize("name", sorted(P.csr_cases()))
def test_csr_from_sorted(name):
    seg, n = P.csr_cases()[name]
    ptr = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
    sd = _t(seg) if len(seg) else None
    _ffi.call("mp_csr_from_sorted_i32", _ffi.ptr(sd), len(seg), n, _ffi.ptr(ptr), _ffi.stream())
    _exact(_np(ptr), P.csr_reference(seg, n), "csr " + name)


@pytest.mark.parametrize("name", sorted(P.sort_cases()))
def test_sort_segments_is_the_stable_argsort(name):
    seg = P.sort_cases()[name]
    m = len(seg)
    nbytes = _ffi.workspace_bytes("mp_sort_workspace_bytes", m)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    sd = _t(seg)
    srt, perm = torch.empty_like(sd), torch.empty_like(sd)
    _ffi.call("mp_sort_segments_i32", _ffi.ptr(sd), m, _ffi.ptr(srt), _ffi.ptr(perm), _ffi.ptr(ws), nbytes, _ffi.stream())
    order = np.argsort(seg, kind="stable")
    _exact(_np(perm), order.astype(np.int32), "perm")
    _exact(_np(srt), seg[order], "sorted ids")


# ============================================================================================== C. Dense family
def _dense(case, bias=True, act=0, misalign=False):
    x, w, b = _t(case["x"]), _t(case["w"]), _t(case["b"]) if bias else None
    if misalign:
        x = _misaligned(x)
    r, k = case["x"].shape
    u = case["w"].shape[1]
    out = _out(r, u)
    _ffi.call("mp_dense_f32", _ffi.ptr(x), r, k, _ffi.ptr(w), _ffi.ptr(b), u, act, P.ALPHA, _ffi.ptr(out), _ffi.stream())
    return _np(out)


@pytest.mark.parametrize("shape", P.dense_triples(), ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("bias", [True, False])
def test_dense_tails(shape, bias):
    case = P.dense_case(*shape)
    assert_rows_close(_dense(case, bias), P.dense_reference(case, np.float32, bias)[0],
                      P.dense_reference(case, np.float64, bias)[0], what="dense %s bias %d" % (shape, bias))


@pytest.mark.parametrize("shape", [(65, 64, 68), (129, 132, 132), (63, 4, 4)])
def test_dense_scalar_build_gives_the_vector_build_bits(shape):
    """A 16-byte-eligible shape from a misaligned x: both builds stage the same tile and issue the same MFMA order."""
    assert P.vec_eligible(shape[1], shape[2])
    case = P.dense_case(*shape)
    aligned = _dense(case)
    _bits(_dense(case, misalign=True), aligned, "dense %s" % (shape,))
    assert_rows_close(aligned, P.dense_reference(case, np.float32)[0], P.dense_reference(case, np.float64)[0])


def _dense_ex(case, bias=True, act=0, in_mode=0, in_act=0, grad_pre=False, addend=None, want_pre=False, misalign=False):
    """``addend``: None, "separate" or "alias" (the addend is the output buffer itself)."""
    x, w, b = _t(case["x"]), _t(case["w"]), _t(case["b"]) if bias else None
    pre_in = _t(case["pre"]) if in_mode == 2 else None
    if misalign:
        x = _misaligned(x)
    gp = _t(case["gpre"]) if grad_pre else None
    r, k = case["x"].shape
    u = case["w"].shape[1]
    out = _t(case["add"]) if addend == "alias" else _out(r, u)
    add = out if addend == "alias" else (_t(case["add"]) if addend == "separate" else None)
    out_pre = _out(r, u) if want_pre else None
    _ffi.call("mp_dense_ex_f32", _ffi.ptr(x), r, k, _ffi.ptr(w), _ffi.ptr(b), u, act, P.ALPHA, in_mode, in_act, P.ALPHA,
              _ffi.ptr(pre_in), _ffi.ptr(add), _ffi.ptr(out_pre), _ffi.ptr(gp), _ffi.ptr(out), _ffi.stream())
    return _np(out), (None if out_pre is None else _np(out_pre))


def _both(case, **kw):
    return P.dense_reference(case, np.float32, **kw), P.dense_reference(case, np.float64, **kw)


@pytest.mark.parametrize("shape", P.DENSE_EX_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("code", sorted(P.ACT_NAMES))
def test_dense_ex_prologue_and_gradient_epilogue(shape, code):
    """in_mode 1 (act(x) staged), in_mode 2 (x * act'(in_pre) staged) and grad_pre (result times in_act'(grad_pre)), each
    on its own, for every activation code."""
    case = P.dense_case(*shape)
    for kw in ({"in_mode": 1, "in_act": code}, {"in_mode": 2, "in_act": code},
               {"act_code": 2, "in_act": code, "grad_pre": True}):
        r32, r64 = _both(case, **kw)
        got, _ = _dense_ex(case, act=kw.get("act_code", 0), in_mode=kw.get("in_mode", 0), in_act=code,
                           grad_pre=kw.get("grad_pre", False))
        assert_rows_close(got, r32[0], r64[0], what="dense_ex %s %s" % (shape, kw))
    if P.vec_eligible(shape[1], shape[2]):
        for mode in (1, 2):
            _bits(_dense_ex(case, in_mode=mode, in_act=code, misalign=True)[0], _dense_ex(case, in_mode=mode, in_act=code)[0],
                  "prologue %d scalar build" % mode)


@pytest.mark.parametrize("shape", P.DENSE_EX_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_dense_ex_out_pre_and_addend(shape):
    case = P.dense_case(*shape)
    r32, r64 = _both(case, act_code=4)
    got, pre = _dense_ex(case, act=4, want_pre=True)
    assert_rows_close(got, r32[0], r64[0], what="dense_ex out next to out_pre")
    assert_rows_close(pre, r32[1], r64[1], what="dense_ex out_pre")
    _bits(got, _dense(case, act=4), "out_pre changes no bit of out")
    r32, r64 = _both(case, act_code=2, addend=True)
    sep, _ = _dense_ex(case, act=2, addend="separate")
    assert_rows_close(sep, r32[0], r64[0], what="dense_ex addend")
    alias, _ = _dense_ex(case, act=2, addend="alias")
    _bits(alias, sep, "addend == out")
    r32, r64 = _both(case, bias=False, act_code=2, in_act=6, grad_pre=True, addend=True)
    got, pre = _dense_ex(case, bias=False, act=2, in_act=6, grad_pre=True, addend="alias", want_pre=True)
    assert_rows_close(got, r32[0], r64[0], what="dense_ex every epilogue form, no bias")
    assert_rows_close(pre, r32[1], r64[1], what="dense_ex out_pre, no bias")


@pytest.mark.parametrize("k,splits", P.SPLITK_CASES)
def test_dense_splitk(k, splits):
    r, u = P.SPLITK_R, P.SPLITK_U
    case = P.dense_case(r, k, u)
    nbytes = _ffi.workspace_bytes("mp_dense_splitk_workspace_bytes", r, u, splits)
    assert nbytes == 4 * r * u * splits and P.splitk_used(k, splits) <= splits
    ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device="cuda")
    x, w, b = _t(case["x"]), _t(case["w"]), _t(case["b"])
    r32, r64 = _both(case, act_code=2)
    for bias in (b, None):
        out = _out(r, u)
        _ffi.call("mp_dense_splitk_f32", _ffi.ptr(x), r, k, _ffi.ptr(w), _ffi.ptr(bias), u, 2, P.ALPHA, splits, _ffi.ptr(ws),
                  nbytes, _ffi.ptr(out), _ffi.stream())
        got = _np(out)
        if bias is None:
            r32, r64 = _both(case, bias=False, act_code=2)
        assert_rows_close(got, r32[0], r64[0], what="split-K K=%d splits=%d" % (k, splits))
        assert_rows_close(got, _dense(case, bias is not None, act=2), r64[0], what="split-K against mp_dense_f32")
    if P.splitk_used(k, splits) == 1:
        _bits(got, _dense(case, False, act=2), "one slice: the k order of mp_dense_f32")


def test_dense_layer_selects_splitk(monkeypatch):
    from gcnn_keras_amd.layers.modules import Dense
    calls = []
    real = _ffi.call

    def spy(name, *args):
        calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(_ffi, "call", spy)
    for (rows, k, u), expect in (((100, 512, 64), True), ((100, 511, 64), False), ((64 * 128, 512, 64), True),
                                 ((64 * 128 + 1, 512, 64), False)):
        assert P.layer_takes_splitk(rows, k, u) == expect
        case = P.dense_case(rows, k, u)
        lay = Dense(u, activation="linear")
        lay.ensure_built((None, None, k))
        lay.set_weights([case["w"], case["b"]])
        del calls[:]
        out = lay(RaggedTensor.from_numpy(case["x"], np.array([0, rows // 2, rows], np.int64)))
        got = _np(out.values)
        gemm = [c for c in calls if c.startswith("mp_dense")]
        assert gemm == ["mp_dense_splitk_f32" if expect else "mp_dense_f32"], gemm
        r32, r64 = _both(case)
        assert_rows_close(got, r32[0], r64[0], what="Dense layer %s" % ((rows, k, u),))


def _rows_call(name, x, *extra):
    xd = _t(x)
    out = _out(*x.shape)
    keep = [_t(e) if isinstance(e, np.ndarray) else e for e in extra]
    args = [_ffi.ptr(e) if (e is None or isinstance(e, torch.Tensor)) else e for e in keep]
    if name == "mp_softmax_rows_grad_f32":
        _ffi.call(name, _ffi.ptr(xd), args[0], x.shape[0], x.shape[1], _ffi.ptr(out), _ffi.stream())
    elif name == "mp_layer_norm_f32":
        _ffi.call(name, _ffi.ptr(xd), x.shape[0], x.shape[1], args[0], args[1], args[2], _ffi.ptr(out), _ffi.stream())
    else:
        _ffi.call(name, _ffi.ptr(xd), x.shape[0], x.shape[1], _ffi.ptr(out), _ffi.stream())
    return _np(out)


@pytest.mark.parametrize("c", P.ROW_WIDTHS)
def test_softmax_rows_and_its_reverse(c):
    case = P.rows_case(c)
    y32, y64 = P.softmax_rows(case["x"], np.float32), P.softmax_rows(case["x"], np.float64)
    got = _rows_call("mp_softmax_rows_f32", case["x"])
    assert_rows_close(got, y32, y64, what="softmax rows C=%d" % c)
    assert np.max(np.abs(got.astype(np.float64).sum(axis=1) - 1)) <= RTOL
    assert_rows_close(_rows_call("mp_softmax_rows_grad_f32", y32, case["g"]), P.softmax_rows_grad(y32, case["g"], np.float32),
                      P.softmax_rows_grad(y32, case["g"], np.float64), what="softmax rows reverse C=%d" % c)


@pytest.mark.parametrize("c", P.ROW_WIDTHS)
def test_layer_norm(c):
    case = P.rows_case(c)
    x = case["x"][1:]                                  # row 0 of the case (entries near 1e4) belongs to the softmax
    for gamma, beta in ((case["gamma"], case["beta"]), (None, case["beta"]), (case["gamma"], None), (None, None)):
        got = _rows_call("mp_layer_norm_f32", x, gamma, beta, ctypes.c_float(1e-3))
        assert_rows_close(got, P.layer_norm(x, gamma, beta, 1e-3, np.float32), P.layer_norm(x, gamma, beta, 1e-3, np.float64),
                          what="layer norm C=%d gamma %d beta %d" % (c, gamma is not None, beta is not None))
        ref_const = np.zeros(c, np.float32) if beta is None else beta
        assert np.max(np.abs(got[0] - ref_const)) <= 1e-5          # the constant row: variance 0


def test_row_kernels_second_grid_stride_trip():
    rows, c = P.ROWS_SECOND_TRIP, 7
    rng = np.random.default_rng(11)
    x, g = rng.normal(size=(rows, c)).astype(np.float32), rng.normal(size=(rows, c)).astype(np.float32)
    y32 = P.softmax_rows(x, np.float32)
    assert_rows_close(_rows_call("mp_softmax_rows_f32", x), y32, P.softmax_rows(x, np.float64), what="softmax, 8200 rows")
    assert_rows_close(_rows_call("mp_softmax_rows_grad_f32", y32, g), P.softmax_rows_grad(y32, g, np.float32),
                      P.softmax_rows_grad(y32, g, np.float64), what="softmax reverse, 8200 rows")
    assert_rows_close(_rows_call("mp_layer_norm_f32", x, None, None, ctypes.c_float(1e-3)),
                      P.layer_norm(x, None, None, 1e-3, np.float32), P.layer_norm(x, None, None, 1e-3, np.float64),
                      what="layer norm, 8200 rows")


# ======================================================================================== D. parameter gradients
def _wgrad(case, with_db=True, short=0, sentinel=None):
    x, g = _t(case["x"]), _t(case["g"])
    r, k = case["x"].shape
    u = case["g"].shape[1]
    nbytes = _ffi.workspace_bytes("mp_dense_wgrad_ws_bytes", r, k, u)
    ws = torch.full((max(nbytes // 4, 1),), float("nan"), dtype=torch.float32, device="cuda")
    dw = _out(k, u) if sentinel is None else torch.full((k, u), sentinel, dtype=torch.float32, device="cuda")
    db = _out(u) if with_db else None
    _ffi.call("mp_dense_wgrad_f32", _ffi.ptr(x), r, k, _ffi.ptr(g), u, _ffi.ptr(dw), _ffi.ptr(db), _ffi.ptr(ws),
              nbytes - short, _ffi.stream())
    torch.cuda.current_stream().synchronize()
    return _np(dw), (None if db is None else _np(db)), nbytes


@pytest.mark.parametrize("shape", P.wgrad_shapes(), ids=lambda s: "%dx%dx%d" % s)
def test_dense_wgrad_across_the_chunk_plan(shape):
    case = P.wgrad_case(*shape)
    (w32, b32), (w64, b64) = P.wgrad_reference(case, np.float32), P.wgrad_reference(case, np.float64)
    dw, db, nbytes = _wgrad(case)
    assert (nbytes == 0) == (P.wgrad_plan(*shape)[1] == 1)
    assert_rows_close(dw, w32, w64, what="wgrad dW %s" % (shape,))
    assert_rows_close(db[None], b32[None], b64[None], what="wgrad db %s" % (shape,))
    dw_only, none, _ = _wgrad(case, with_db=False)
    _bits(dw_only, dw, "dW without db")
    again, db_again, _ = _wgrad(case)
    _bits(again, dw, "second run")
    _bits(db_again, db, "second run, db")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        other, db_other, _ = _wgrad(case)
    torch.cuda.synchronize()
    _bits(other, dw, "second stream")
    _bits(db_other, db, "second stream, db")


def test_dense_wgrad_short_workspace_is_refused():
    shape = (1025, 64, 64)
    assert P.wgrad_plan(*shape)[1] > 1
    case = P.wgrad_case(*shape)
    with pytest.raises(ValueError):
        _wgrad(case, short=1, sentinel=7.0)
    x, g = _t(case["x"]), _t(case["g"])
    nbytes = _ffi.workspace_bytes("mp_dense_wgrad_ws_bytes", *shape)
    ws = torch.zeros(nbytes // 4, dtype=torch.float32, device="cuda")
    dw = torch.full((64, 64), 7.0, dtype=torch.float32, device="cuda")
    rc = _ffi.lib().mp_dense_wgrad_f32(_ffi.ptr(x), 1025, 64, _ffi.ptr(g), 64, _ffi.ptr(dw), None, _ffi.ptr(ws), nbytes - 1,
                                       _ffi.stream())
    torch.cuda.synchronize()
    assert rc == _ffi.MP_EINVAL and bool((dw == 7.0).all()) and not bool(ws.any())


@pytest.mark.parametrize("n,vocab,dim", P.EMBED_GRAD_SHAPES)
def test_embedding_grad_is_the_node_order_sum(n, vocab, dim):
    case = P.embedding_grad_case(n, vocab, dim)
    nbytes = _ffi.workspace_bytes("mp_embedding_grad_ws_bytes", n, vocab)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    numbers, g = _t(case["numbers"]), _t(case["g"])
    out = _out(vocab, dim)
    _ffi.call("mp_embedding_grad_f32", _ffi.ptr(numbers), n, _ffi.ptr(g), vocab, dim, _ffi.ptr(ws), nbytes, _ffi.ptr(out),
              _ffi.stream())
    _bits(_np(out), P.embedding_grad_reference(case, vocab, np.float32), "embedding grad")


# ==================================================================================================== E. GCN tiles
def _gcn_model(case):
    from gcnn_keras_amd.literature import GCN
    model = GCN.make_model(
        inputs=[{"shape": (None, case["feats"]), "name": "node_attributes", "dtype": "float32", "ragged": True},
                {"shape": (None, 1), "name": "edge_weights", "dtype": "float32", "ragged": True},
                {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True}],
        gcn_args={"units": case["units"], "use_bias": True, "activation": "relu", "pooling_method": "sum"},
        depth=2, output_embedding="node", output_to_tensor=False,
        output_mlp={"use_bias": True, "units": list(case["out_units"]), "activation": ["relu", "linear"]})
    model.set_weights(list(case["params"].values()))
    assert model.fused is not None
    return model


def _gcn_oracle(case, dtype):
    return ko.gcn_forward(ko.to_dtype(case["params"], dtype), ko.R(case["attrs"].astype(dtype), case["ns"]),
                          ko.R(case["w"].astype(dtype), case["es"]), ko.R(case["idx"], case["es"]), depth=2,
                          output_mlp_act=("relu", "linear")).values


def _check_gcn(case, what, table):
    model = _gcn_model(case)
    ins = [RaggedTensor.from_numpy(case["attrs"], case["ns"]), RaggedTensor.from_numpy(case["w"], case["es"]),
           RaggedTensor.from_numpy(case["idx"], case["es"])]
    first = _np(model(ins).values)
    assert model.fused.last == "eager"
    slot = model.fused.slot_of(ins)
    starts = P.gcn_tiles(case["deg"])
    assert (slot.tile_start is not None) == table == (starts is not None)
    if table:
        _exact(_np(slot.tile_start), starts.astype(np.int32), "tile table")
        assert slot.n_tiles == len(starts) - 1 and np.any(np.diff(_np(slot.tile_start)) < 16)
    replay = _np(model(ins).values)
    assert model.fused.last == "graph"
    _bits(replay, first, "graph replay")
    layers = _np(model(ins, fused=False).values)
    r32, r64 = _gcn_oracle(case, np.float32), _gcn_oracle(case, np.float64)
    assert_rows_close(first, r32, r64, what=what)
    assert_rows_close(layers, r32, r64, what=what + " (layer sequence)")
    bar = max(RTOL, min(2 * rowwise_rel(r32, r64), BAR_CAP))
    assert rowwise_rel(first, layers) <= 2 * bar, "%s: fused vs layer sequence %.3g (bar %.3g)" % (
        what, rowwise_rel(first, layers), 2 * bar)


@pytest.mark.parametrize("units,hub", P.GCN_HUB_CASES)
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_gcn_hub_walks_several_edge_windows(units, hub, order):
    """One receiver with more edges than a window holds (768 at 128 units, 1792 at 64 and 32): two windows with a second
    of one edge, and three windows; the hub is a tile of its own in the tile table."""
    deg = P.gcn_degrees(40, seed=hub, hub=hub)
    assert P.gcn_windows(deg, units) == {769: 2, 1793: 2, 3600: 3}[hub]
    _check_gcn(P.gcn_case(deg, 20, units, order=order), "GCN hub %d edges, %d units, %s" % (hub, units, order), table=True)


@pytest.mark.parametrize("busiest,table", [(512, False), (513, True)])
def test_gcn_uniform_tile_boundary(busiest, table):
    _check_gcn(P.gcn_case(P.gcn_uniform_degrees(busiest), 20, 64), "GCN uniform tile of %d edges" % busiest, table=table)


@pytest.mark.parametrize("n,feats", [(17, 20), (33, 20), (20, 528), (20, 529)])
def test_gcn_last_tile_of_one_row_and_long_input_rows(n, feats):
    """17 and 33 nodes: the last tile holds one row.  528 and 529 input features: 33 full k blocks, nine for the first
    wave - a second trip of the eight-deep pipeline loop - without and with the ragged last block."""
    deg = P.gcn_degrees(n, seed={17: 1, 33: 2, 20: 3}[n])
    _check_gcn(P.gcn_case(deg, feats, 64), "GCN %d nodes, %d features" % (n, feats), table=False)
