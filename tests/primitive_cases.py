"""Cases off the tiny random graphs for the layer-path kernels: segment reductions, gathers, index preparation, the Dense
family, the weight gradients and the GCN tile kernel.

``tests/test_gpu_layers.py`` feeds these kernels at most 9 nodes and 40 edges per graph; the kernels branch on segment
length (16- and 8-row rounds), on the number of work items against the grid cap (524 288 threads), on the graph count
against the LDS search (1023), on k / row tails of the MFMA tiles, on the chunk plan of the weight gradient and on the
edge window of the GCN tile.  This module holds seeded generators that reach those branches and NumPy restatements (float32
in the kernel's accumulation order where the test asks for equal bits, float64 as the truth), without any engine import:
tests/test_primitive_cases.py checks on the CPU that every generator delivers the boundary it claims and that each float32
restatement is inside half the cap tests/test_gpu_primitive_edges.py applies."""
import numpy as np

GRID_CAP = 2048 * 256          # mp::grid_for: at most 2048 blocks of 256 threads; above this a grid-stride loop runs twice
PREP_LDS_GRAPHS = 1023         # csrc/mp_edge_prepare.h: batches up to this many graphs search their splits in LDS
FLAG_OOB, FLAG_UNSORTED_COL0, FLAG_UNSORTED_COL1 = 1, 2, 4
SUM, MEAN, MAX, MIN = 0, 1, 2, 3

# ------------------------------------------------------------------------------------------------------ activations
ACT_NAMES = {0: "linear", 1: "relu", 2: "kgcnn>shifted_softplus", 3: "softplus", 4: "swish", 5: "sigmoid", 6: "tanh",
             7: "kgcnn>leaky_relu", 8: "kgcnn>softplus2", 9: "selu"}
ALPHA = 0.05
_SELU_SCALE, _SELU_ALPHA = 1.05070098, 1.67326324


def _sigmoid(x):
    t = x.dtype.type
    with np.errstate(over="ignore"):
        return (t(1) / (t(1) + np.exp(-x))).astype(x.dtype)


def act(code, x, alpha=ALPHA):
    """Activation ``code`` of include/mpengine/core.h in the dtype of ``x``."""
    x = np.asarray(x)
    t = x.dtype.type
    if code == 0:
        return x
    if code == 1:
        return np.maximum(x, t(0))
    if code == 2:
        return (np.logaddexp(t(0), x) - np.log(t(2))).astype(x.dtype)
    if code == 3:
        return np.logaddexp(t(0), x).astype(x.dtype)
    if code == 4:
        return x * _sigmoid(x)
    if code == 5:
        return _sigmoid(x)
    if code == 6:
        return np.tanh(x)
    if code == 7:
        return np.where(x >= 0, x, t(alpha) * x).astype(x.dtype)
    if code == 8:
        return (np.maximum(x, t(0)) + np.log(t(0.5) * np.exp(-np.abs(x)) + t(0.5))).astype(x.dtype)
    if code == 9:
        return (t(_SELU_SCALE) * np.where(x > 0, x, t(_SELU_ALPHA) * (np.exp(np.minimum(x, t(0))) - t(1)))).astype(x.dtype)
    raise ValueError(code)


def act_grad(code, x, alpha=ALPHA):
    """d act / d x of activation ``code`` (what the reverse pass multiplies by)."""
    x = np.asarray(x)
    t = x.dtype.type
    if code == 0:
        return np.ones_like(x)
    if code == 1:
        return (x > 0).astype(x.dtype)
    if code in (2, 3, 8):
        return _sigmoid(x)
    if code == 4:
        s = _sigmoid(x)
        return s + x * s * (t(1) - s)
    if code == 5:
        s = _sigmoid(x)
        return s * (t(1) - s)
    if code == 6:
        th = np.tanh(x)
        return t(1) - th * th
    if code == 7:
        return np.where(x >= 0, t(1), t(alpha)).astype(x.dtype)
    if code == 9:
        return (t(_SELU_SCALE) * np.where(x > 0, t(1), t(_SELU_ALPHA) * np.exp(np.minimum(x, t(0))))).astype(x.dtype)
    raise ValueError(code)


# ------------------------------------------------------------------------------------- A. segment reductions (CSR)
# in order: empty rows at the front, inside and at the end; 1..15 run 8-row rounds only (remainders 1, 7, 0, 1, 7 of 8);
# 16..33 take one or two 16-row rounds followed by 0..2 8-row rounds; 129 = 8 x 16 + 1 (the first-element rule is tested
# inside the ninth round), 1000 = 62 x 16 + 8
SEGMENT_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 0, 129, 1000, 0)
SEGMENT_WIDTHS = (1, 3, 4, 128, 130)
ZERO_WEIGHT_SEGMENT = 3        # the 8-row segment: weights +-0.5 alternate, their float sum is exactly 0
GATHER_ROWS = 37               # rows of the table the gather-on-read variants read


def rounds_of(length):
    """(16-row rounds, 8-row rounds, rows of the last round) the CSR kernel takes for a segment of ``length`` rows."""
    r16 = length // 16
    left = length - 16 * r16
    r8 = -(-left // 8)
    last = 0 if length == 0 else (left - 8 * (r8 - 1) if r8 else 16)
    return r16, r8, last


def segment_ptr(lengths=SEGMENT_LENGTHS, dtype=np.int32):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(dtype)


def segment_case(width, seed=0, perm=False, gather=False, weight=False, data="normal", lengths=SEGMENT_LENGTHS):
    """One CSR reduce call.  ``perm``: the rows come in shuffled edge order with the stable argsort of their receivers;
    ``gather``: rows are ``x[send[e]]`` with a few sender ids below 0 and at or above the table size (clamped by the
    kernel); ``weight``: one weight per edge (the ``ZERO_WEIGHT_SEGMENT`` sums to exactly 0).  ``data``: "normal",
    "negative" (all below 0, each segment's largest value in its last row), "positive" (the mirror image, for min) or
    "grid": rows on a grid of 1/64 in -2..2 and weights on a grid of 1/16 in 1/8..1, whose products and 1000-row sums are
    exact in float32 - the cases held to the 1e-6 / 2e-6 bars of tests/test_gpu_layers.py (mean, weighted), where the
    float32 sum of 1000 normal deviates is itself 3e-6 of the row away from float64."""
    rng = np.random.default_rng(1000 * seed + width)
    ptr = segment_ptr(lengths)
    n, m = len(lengths), int(ptr[-1])
    recv_sorted = np.repeat(np.arange(n), lengths)
    if perm:
        recv = recv_sorted[rng.permutation(m)]
        order = np.argsort(recv, kind="stable")
    else:
        recv, order = recv_sorted, np.arange(m)
    case = {"ptr": ptr, "M": m, "N": n, "width": width, "recv": recv.astype(np.int32),
            "perm": order.astype(np.int32) if perm else None, "order": order, "send": None, "weight": None}
    if gather:
        table = rng.integers(-128, 129, size=(GATHER_ROWS, width)) / 64.0 if data == "grid" else \
            rng.normal(size=(GATHER_ROWS, width))
        case["x"] = table.astype(np.float32)
        send = rng.integers(0, GATHER_ROWS, size=m)
        send[rng.choice(m, size=6, replace=False)] = [-1, -7, GATHER_ROWS, GATHER_ROWS + 5, -2, GATHER_ROWS + 1]
        case["send"] = send.astype(np.int32)
    else:
        if data == "normal":
            rows = rng.normal(size=(m, width))
        elif data == "grid":
            rows = rng.integers(-128, 129, size=(m, width)) / 64.0
        else:
            rows = -rng.uniform(1.0, 2.0, size=(m, width))
            rows[ptr[1:][np.asarray(lengths) > 0] - 1] = -0.5          # the last row of every segment holds its maximum
            if data == "positive":
                rows = -rows
        x = np.empty((m, width), np.float32)
        x[order] = rows.astype(np.float32)                              # rows[k] is the k-th row in receiver order
        case["x"] = x
    if weight:
        w = rng.integers(2, 17, size=m) / 16.0 if data == "grid" else rng.uniform(0.1, 1.0, size=m)
        lo, hi = int(ptr[ZERO_WEIGHT_SEGMENT]), int(ptr[ZERO_WEIGHT_SEGMENT + 1])
        w[lo:hi] = np.where(np.arange(hi - lo) % 2 == 0, 0.5, -0.5)
        we = np.empty(m, np.float32)
        we[order] = w.astype(np.float32)
        case["weight"] = we
    return case


def fold_segments(rows, ptr, op, dtype):
    """Segment reduce of ``rows`` (already in receiver order) accumulated in edge order in ``dtype``: vectorised over the
    segments, a loop over the position inside the segment.  The first row initialises the accumulator; empty segments
    give 0."""
    rows = np.asarray(rows, dtype)
    ptr = np.asarray(ptr, np.int64)
    lens = np.diff(ptr)
    out = np.zeros((len(lens),) + rows.shape[1:], dtype)
    for p in range(int(lens.max()) if len(lens) else 0):
        sel = np.nonzero(lens > p)[0]
        r = rows[ptr[sel] + p]
        if p == 0:
            out[sel] = r
        elif op == MAX:
            out[sel] = np.maximum(out[sel], r)
        elif op == MIN:
            out[sel] = np.minimum(out[sel], r)
        else:
            out[sel] = out[sel] + r
    if op == MEAN:
        nz = lens > 0
        out[nz] = out[nz] / lens[nz].astype(dtype).reshape((-1,) + (1,) * (rows.ndim - 1))
    return out


def segment_rows(case, dtype):
    """The rows a case reduces, in receiver order (after the permutation, the gather with clamped ids and the weight)."""
    order = case["order"]
    if case["send"] is not None:
        rows = case["x"][np.clip(case["send"][order].astype(np.int64), 0, GATHER_ROWS - 1)]
    else:
        rows = case["x"][order]
    rows = rows.astype(dtype)
    if case["weight"] is not None:
        rows = rows * case["weight"][order].astype(dtype)[:, None]
    return rows


def segment_reference(case, op, dtype, normalize=False, act_code=0):
    out = fold_segments(segment_rows(case, dtype), case["ptr"], op, dtype)
    if normalize and case["weight"] is not None:
        wsum = fold_segments(case["weight"][case["order"]].astype(dtype)[:, None], case["ptr"], SUM, dtype)
        with np.errstate(divide="ignore", invalid="ignore"):
            out = np.where(wsum == 0, dtype(0), out / wsum).astype(dtype)
    return act(act_code, out)


POOL_GRAPH_ROWS = (0, 1, 16, 17, 5000, 0)
POOL_MANY_GRAPHS, POOL_MANY_WIDTH = 16400, 128       # 16 400 x 32 chunks = 524 800 work items: a second grid-stride trip


def pool_case(width, seed=0):
    rng = np.random.default_rng(50 + seed + width)
    splits = segment_ptr(POOL_GRAPH_ROWS, np.int64)
    n = int(splits[-1])
    return {"splits": splits, "x": rng.normal(size=(n, width)).astype(np.float32),
            "grid": (rng.integers(-128, 129, size=(n, width)) / 64.0).astype(np.float32),     # as segment_case's "grid"
            "weight": (rng.integers(2, 17, size=n) / 16.0).astype(np.float32)}


def softmax_case(perm, seed=0, width=3):
    """Segment softmax over ``SEGMENT_LENGTHS``: column 0 holds values near 1e4, the 16-row segment holds equal values."""
    case = segment_case(width, seed=seed + 7, perm=perm)
    rows = case["x"][case["order"]].copy()
    rows[:, 0] += np.float32(1e4)
    lo, hi = int(case["ptr"][6]), int(case["ptr"][7])
    rows[lo:hi] = np.float32(0.7)
    case["x"][case["order"]] = rows
    case["equal_segment"] = 6
    return case


def segment_softmax_reference(case, dtype):
    """exp(a - max_seg) / sum_seg exp(a - max_seg) per segment and column, rows back in edge order."""
    rows = case["x"][case["order"]].astype(dtype)
    ptr = case["ptr"].astype(np.int64)
    ids = np.repeat(np.arange(case["N"]), np.diff(ptr))
    mx = fold_segments(rows, ptr, MAX, dtype)
    e = np.exp(rows - mx[ids])
    s = fold_segments(e, ptr, SUM, dtype)
    out = np.empty_like(e)
    out[case["order"]] = e / s[ids]
    return out


RELATIONAL_HUB = 1000


def relational_case(width=4, seed=0, nodes=12, relations=3):
    """Unsorted relational scatter: mixed signs with some -0.0, relation ids of -1 and ``relations`` (skipped), a hub
    (node 5, relation 1) slot of ``RELATIONAL_HUB`` edges, slots that only receive negative (max) or positive (min)
    values, and slots that receive nothing."""
    rng = np.random.default_rng(90 + seed + width)
    m = 600
    recv = rng.integers(0, nodes - 1, size=m)                  # the last node receives nothing
    rel = rng.integers(-1, relations + 1, size=m)
    recv = np.concatenate([recv, np.full(RELATIONAL_HUB, 5)])
    rel = np.concatenate([rel, np.full(RELATIONAL_HUB, 1)])
    val = rng.normal(size=(len(recv), width)).astype(np.float32)
    val[rng.choice(len(recv), size=20, replace=False)] = np.float32(-0.0)
    val[(recv == 2) & (rel == 0)] = -np.abs(val[(recv == 2) & (rel == 0)]) - np.float32(0.25)     # all-negative slot
    val[(recv == 3) & (rel == 2)] = np.abs(val[(recv == 3) & (rel == 2)]) + np.float32(0.25)      # all-positive slot
    p = rng.permutation(len(recv))
    return {"recv": recv[p].astype(np.int32), "rel": rel[p].astype(np.int32), "val": val[p], "N": nodes, "R": relations}


# ---------------------------------------------------------------------------------------- B. gathers and index work
GATHER_TOTALS = (GRID_CAP - 1, GRID_CAP, GRID_CAP + 1, 4 * GRID_CAP + 37)
GATHER_TABLE = 1000


def gather_case(m, ncols, width, colsel, seed=0, k=4):
    """``mp_gather_rows_f32`` operands: a table of ``GATHER_TABLE`` rows, ``k`` prepared int32 columns of ``m`` ids with
    -1 and the table size among them (read as zeros), and the column selection."""
    rng = np.random.default_rng(seed + m % 9973 + 17 * width + ncols)
    cols = rng.integers(0, GATHER_TABLE, size=(k, m)).astype(np.int32)
    bad = rng.choice(m, size=min(m, 8), replace=False)
    cols[:, bad[::2]] = -1
    cols[:, bad[1::2]] = GATHER_TABLE
    return {"x": rng.normal(size=(GATHER_TABLE, width)).astype(np.float32), "cols": cols, "colsel": list(colsel),
            "M": m, "ncols": ncols, "width": width}


def gather_items(case, vector):
    """Work items of the launch: (edge, selected column, 16-byte chunk) in the float4 build, one per float otherwise."""
    per_row = case["width"] // 4 if vector else case["width"]
    return case["M"] * case["ncols"] * per_row


def take_rows(x, ids):
    """x[ids] with ids outside the table read as zero rows (TF-GPU gather semantics)."""
    ids = np.asarray(ids, np.int64)
    ok = (ids >= 0) & (ids < len(x))
    out = x[np.where(ok, ids, 0)]
    out[~ok] = 0
    return out


def gather_reference(case):
    ids = case["cols"][np.asarray(case["colsel"])].T            # (M, ncols)
    return take_rows(case["x"], ids)                            # (M, ncols, width)


INDEX_LONG = GRID_CAP + 67        # edges of the long batch: the prefetch of the next grid-stride trip is live
INDEX_CASES = tuple((g, m) for g in (1, 1023, 1024, 1025) for m in (1, 63, 64, 65)) + ((1, INDEX_LONG), (1025, INDEX_LONG))


def batch_splits(g, m, seed, max_nodes=5):
    """Node and edge row_splits of ``g`` graphs holding ``m`` edges: with three or more graphs the first, the middle and
    the last one are empty (no nodes, no edges); every other graph has 2..``max_nodes`` nodes, and the last of them at
    least two edges (if there are two)."""
    rng = np.random.default_rng(seed + 31 * g + m % 1009)
    n_len = rng.integers(2, max_nodes + 1, size=g)
    if g >= 3:
        n_len[[0, g // 2, g - 1]] = 0
    live = np.nonzero(n_len > 0)[0]
    e_len = np.zeros(g, np.int64)
    e_len[live[-1]] = min(m, 2)
    np.add.at(e_len, rng.choice(live, size=m - min(m, 2)), 1)
    ns = np.concatenate([[0], np.cumsum(n_len)]).astype(np.int64)
    es = np.concatenate([[0], np.cumsum(e_len)]).astype(np.int64)
    return ns, es


def index_batch(g, m, k=2, seed=0, max_nodes=5):
    """Sample-level ``(m, k)`` int64 ids, every column ascending inside every graph: the only descents of the local ids
    are across graph boundaries."""
    ns, es = batch_splits(g, m, seed, max_nodes)
    rng = np.random.default_rng(seed + 7 * g + m % 1013 + k)
    graph = np.repeat(np.arange(g), np.diff(es))
    n_of = np.diff(ns)[graph]
    idx = np.floor(rng.random((m, k)) * n_of[:, None]).astype(np.int64)
    for c in range(k):
        idx[:, c] = idx[np.lexsort((idx[:, c], graph)), c]
    return {"idx": idx, "node_splits": ns, "edge_splits": es, "G": g, "M": m, "K": k, "N": int(ns[-1]), "graph": graph}


def with_descent(batch, col):
    """A copy with one descent inside a graph in column ``col`` (the last graph that has two edges and two nodes), or
    None if no graph has room for one."""
    es, ns = batch["edge_splits"], batch["node_splits"]
    ok = np.nonzero((np.diff(es) >= 2) & (np.diff(ns) >= 2))[0]
    if ok.size == 0:
        return None
    g = int(ok[-1])
    e = int(es[g + 1]) - 2
    out = dict(batch, idx=batch["idx"].copy())
    out["idx"][e, col] = ns[g + 1] - ns[g] - 1
    out["idx"][e + 1, col] = 0
    return out


def with_oob(batch, col):
    """A copy whose last edge holds, in column ``col``, an id equal to its graph's node count."""
    out = dict(batch, idx=batch["idx"].copy())
    g = int(batch["graph"][-1])
    out["idx"][-1, col] = batch["node_splits"][g + 1] - batch["node_splits"][g]
    return out


def index_reference(batch):
    """(cols (K, M) int32 of batch-level ids, flags) of ``mp_index_prepare_i64``: ids clamped into their graph, the
    sortedness of the first two columns judged on the batch-level ids of consecutive edges."""
    idx, ns, graph = batch["idx"], batch["node_splits"], batch["graph"]
    base, n_of = ns[graph], np.diff(ns)[graph]
    bad = (idx < 0) | (idx >= n_of[:, None])
    flags = FLAG_OOB if bad.any() else 0
    shifted = np.clip(idx, 0, np.maximum(n_of - 1, 0)[:, None]) + base[:, None]
    raw = idx + base[:, None]
    for c, bit in zip(range(min(batch["K"], 2)), (FLAG_UNSORTED_COL0, FLAG_UNSORTED_COL1)):
        if np.any(raw[:-1, c] > shifted[1:, c]):
            flags |= bit
    return np.ascontiguousarray(shifted.T).astype(np.int32), flags


def local_descents_across_graphs(batch, col):
    """Number of places where the sample-level id of column ``col`` descends from one edge to the next."""
    return int(np.sum(np.diff(batch["idx"][:, col]) < 0))


def csr_cases():
    """name -> (sorted int32 segment ids, N) for ``mp_csr_from_sorted_i32``."""
    rng = np.random.default_rng(5)
    return {
        "gaps": (np.sort(rng.choice([0, 3, 4, 9, 17, 18, 30], size=200)).astype(np.int32), 33),
        "one-segment": (np.full(700, 4, np.int32), 9),
        "empty": (np.zeros(0, np.int32), 5),
        "above-n": (np.sort(np.concatenate([rng.integers(0, 6, size=40), [6, 9, 9]])).astype(np.int32), 6),
        "second-trip": (np.sort(rng.integers(0, 50, size=GRID_CAP + 5)).astype(np.int32), 50),
    }


def csr_reference(seg, n):
    return np.searchsorted(np.minimum(seg, n), np.arange(n + 1), side="left").astype(np.int32)


def sort_cases():
    rng = np.random.default_rng(6)
    return {"one": np.array([3], np.int32), "few-keys": rng.choice([0, 2, 5, 11, 4000], size=70000).astype(np.int32)}


# ------------------------------------------------------------------------------------------------- C. Dense family
DENSE_R = (1, 63, 64, 65, 129)
DENSE_K = (1, 2, 3, 4, 63, 64, 65, 66, 130, 132)
DENSE_U = (1, 3, 4, 63, 64, 65, 68, 132)


def dense_triples():
    """40 (R, K, U): every R eight times, every K four times, every U five times; K and U advance at different rates so
    that 16-byte-eligible pairs (both multiples of 4) and scalar pairs both occur."""
    return [(DENSE_R[i % 5], DENSE_K[i % 10], DENSE_U[(i + i // 8) % 8]) for i in range(40)]


def vec_eligible(k, u):
    return k % 4 == 0 and u % 4 == 0


def glorot(rng, fan_in, fan_out):
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-lim, lim, size=(fan_in, fan_out)).astype(np.float32)


def dense_case(r, k, u, seed=0):
    """Operands of one Dense call.  An output row of fewer than four entries is a cancelled sum measured against itself
    (float32 is then 3e-5 of the row from float64 whoever computes it): such shapes get operands of one sign."""
    rng = np.random.default_rng(seed + 1000003 * r + 1009 * k + u)
    x, w = rng.normal(size=(r, k)).astype(np.float32), glorot(rng, k, u)
    if u < 4:
        x, w = np.abs(x) + np.float32(0.25), np.abs(w)
    return {"x": x, "w": w,
            "b": rng.uniform(-0.1, 0.1, size=u).astype(np.float32),
            "pre": rng.normal(size=(r, k)).astype(np.float32),        # in_pre of prologue mode 2
            "gpre": rng.normal(size=(r, u)).astype(np.float32),       # grad_pre of the epilogue
            "add": rng.normal(size=(r, u)).astype(np.float32)}        # addend


def dense_reference(case, dtype, bias=True, act_code=0, in_mode=0, in_act=0, grad_pre=False, addend=False):
    """(out, pre-activation) of mp_dense_ex_f32 in ``dtype``."""
    x = case["x"].astype(dtype)
    if in_mode == 1:
        x = act(in_act, x)
    elif in_mode == 2:
        x = x * act_grad(in_act, case["pre"].astype(dtype))
    pre = np.matmul(x, case["w"].astype(dtype))
    if bias:
        pre = pre + case["b"].astype(dtype)
    out = act(act_code, pre)
    if grad_pre:
        out = out * act_grad(in_act, case["gpre"].astype(dtype))
    if addend:
        out = out + case["add"].astype(dtype)
    return out.astype(dtype), pre.astype(dtype)


DENSE_EX_SHAPES = ((65, 66, 68), (65, 128, 384))
SPLITK_CASES = ((64, 4), (100, 64), (1433, 3), (1433, 11), (512, 64))
SPLITK_R, SPLITK_U = 70, 68


def splitk_used(k, splits, bk=64):
    """Slices mp_dense_splitk_f32 launches: the k range of a slice is a multiple of the k tile, trailing empty slices are
    dropped."""
    kchunk = -(-(-(-k // splits)) // bk) * bk
    return -(-k // kchunk)


def layer_takes_splitk(rows, k, u):
    """The choice of layers/modules.py: few 64 x 64 output tiles and a long contraction."""
    return -(-rows // 64) * -(-u // 64) <= 128 and k >= 512


ROW_WIDTHS = (1, 7, 63, 64, 65, 129, 1000)
ROWS_SECOND_TRIP = GRID_CAP // 64 + 8       # one wave per row: this many rows need a second grid-stride trip


def rows_case(c, seed=0, rows=9):
    """Row-wise kernels: row 0 has entries near 1e4, row 1 is constant (variance 0)."""
    rng = np.random.default_rng(seed + c)
    x = rng.normal(size=(rows, c)).astype(np.float32)
    x[0] += np.float32(1e4)
    x[1] = np.float32(0.5)
    return {"x": x, "g": rng.normal(size=(rows, c)).astype(np.float32),
            "gamma": rng.uniform(0.5, 1.5, size=c).astype(np.float32),
            "beta": rng.uniform(-0.5, 0.5, size=c).astype(np.float32)}


def softmax_rows(x, dtype):
    x = np.asarray(x, dtype)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(dtype)


def softmax_rows_grad(y, g, dtype):
    y, g = np.asarray(y, dtype), np.asarray(g, dtype)
    return (y * (g - np.sum(g * y, axis=1, keepdims=True))).astype(dtype)


def layer_norm(x, gamma, beta, eps, dtype):
    x = np.asarray(x, dtype)
    mean = x.mean(axis=1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=1, keepdims=True)
    out = (x - mean) / np.sqrt(var + dtype(eps))
    if gamma is not None:
        out = out * gamma.astype(dtype)
    if beta is not None:
        out = out + beta.astype(dtype)
    return out.astype(dtype)


# ------------------------------------------------------------------------------------------- D. parameter gradients
WGRAD_R = (1, 31, 32, 33, 1000, 1025, 16385)
WGRAD_KU = ((1, 1), (3, 7), (4, 4), (64, 64), (65, 63), (68, 132), (128, 1))


def wgrad_plan(r, k, u, wt=64, br=32, target=512, max_chunks=512):
    """(rows_per_chunk, chunks) of csrc/mp_wgrad.hip's plan_chunks."""
    tiles = -(-k // wt) * -(-u // wt)
    stages = -(-r // br)
    c = max(1, min(-(-target // tiles), max_chunks, stages))
    rows_per_chunk = -(-stages // c) * br
    return rows_per_chunk, -(-r // rows_per_chunk)


def wgrad_shapes():
    """A covering subset: every R with two or three of the (K, U) pairs, every pair at least twice."""
    out = []
    for i, r in enumerate(WGRAD_R):
        for j in range(3):
            out.append((r,) + WGRAD_KU[(3 * i + j) % len(WGRAD_KU)])
    return out


def wgrad_case(r, k, u, seed=0):
    """As ``dense_case``: a dW row of fewer than four entries gets operands of one sign."""
    rng = np.random.default_rng(seed + 7919 * r + 101 * k + u)
    x, g = rng.normal(size=(r, k)).astype(np.float32), rng.normal(size=(r, u)).astype(np.float32)
    if u < 4:
        x, g = np.abs(x) + np.float32(0.25), np.abs(g) + np.float32(0.25)
    return {"x": x, "g": g}


def wgrad_reference(case, dtype):
    x, g = case["x"].astype(dtype), case["g"].astype(dtype)
    return np.matmul(x.T, g).astype(dtype), g.sum(axis=0).astype(dtype)


EMBED_GRAD_SHAPES = ((1, 1, 1), (1, 95, 64), (5000, 1, 130), (5000, 95, 1), (5000, 95, 64), (5000, 95, 130))
EMBED_HUB_ROWS = 4000


def embedding_grad_case(n, vocab, dim, seed=0):
    """Node numbers as floats: with 5000 nodes one type (0 of a one-row table, else 6) holds ``EMBED_HUB_ROWS`` rows; -1,
    ``vocab`` and fractions (truncated) are among the rest."""
    rng = np.random.default_rng(seed + n + 13 * vocab + dim)
    if n == 1:
        numbers = np.array([0.0 if vocab == 1 else 6.9], np.float32)
    else:
        hub = 0 if vocab == 1 else 6
        rest = rng.integers(-1, vocab + 1, size=n - EMBED_HUB_ROWS).astype(np.float64)
        rest[rest == hub] = vocab                      # the hub type holds exactly EMBED_HUB_ROWS rows
        rest[::7] += 0.9 * (rest[::7] >= 0)            # 5.9 truncates to 5
        numbers = np.concatenate([np.full(EMBED_HUB_ROWS, hub + (0.5 if vocab > 1 else 0.0)), rest])
        numbers = numbers[rng.permutation(n)].astype(np.float32)
    return {"numbers": numbers, "g": rng.normal(size=(n, dim)).astype(np.float32), "hub": 0 if vocab == 1 else 6}


def embedding_ids(numbers, vocab):
    """Keras' int32 cast (truncation); numbers outside the table go to the extra id ``vocab``."""
    ids = np.trunc(numbers.astype(np.float64)).astype(np.int64)
    return np.where((ids >= 0) & (ids < vocab), ids, vocab)


def embedding_grad_reference(case, vocab, dtype):
    ids = embedding_ids(case["numbers"], vocab)
    order = np.argsort(ids, kind="stable")
    ptr = np.searchsorted(ids[order], np.arange(vocab + 1), side="left")
    return fold_segments(case["g"][order], ptr, SUM, dtype)


# ----------------------------------------------------------------------------------------------------- E. GCN tiles
GCN_TILE_NODES = 16
GCN_TILE_EDGES = 256           # fused_gcn.FusedGcn.TILE_EDGES
GCN_ECAP = {128: 768, 64: 1792, 32: 1792}        # csrc/mp_gcn.hip: edges per window of the aggregate launch
GCN_HUB_CASES = ((128, 769), (64, 1793), (64, 3600), (32, 1793), (32, 3600))      # (units, edges into node 5)
GCN_HUB_NODE = 5


def gcn_degrees(n, seed, hub=None):
    """In-degrees of ``n`` nodes: 0..6, the first and the last node isolated, ``hub`` edges into ``GCN_HUB_NODE``."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 7, size=n)
    deg[[0, n - 1]] = 0
    if hub is not None:
        deg[GCN_HUB_NODE] = hub
    return deg


def gcn_uniform_degrees(busiest):
    """40 nodes whose first uniform tile (nodes 0..15) holds exactly ``busiest`` edges; the other nodes have 0..6."""
    deg = gcn_degrees(40, seed=busiest)
    deg[:16] = busiest // 16
    deg[3] += busiest - int(deg[:16].sum())
    return deg


def gcn_case(deg, feats, units, order="sorted", seed=0, out_units=(16, 3)):
    """One graph for GCN.make_model(depth=2, relu, sum pooling; output MLP relu -> linear): node attributes, edges
    ``[receiver, sender]`` sorted by receiver or shuffled, weights in 0.05..1, and Glorot weights with random biases under
    the keys of ``synth.gcn_params``."""
    deg = np.asarray(deg)
    n = len(deg)
    rng = np.random.default_rng(seed + 3 * n + feats + units + int(deg.sum()))
    recv = np.repeat(np.arange(n), deg)
    idx = np.stack([recv, rng.integers(0, n, size=len(recv))], axis=1).astype(np.int64)
    w = rng.uniform(0.05, 1.0, size=(len(recv), 1)).astype(np.float32)
    if order == "shuffled":
        p = rng.permutation(len(recv))
        idx, w = idx[p], w[p]
    params = {"dense0/kernel": glorot(rng, feats, units), "dense0/bias": rng.uniform(-0.1, 0.1, units).astype(np.float32)}
    for i in range(2):
        params["gcn%d/kernel" % i] = glorot(rng, units, units)
        params["gcn%d/bias" % i] = rng.uniform(-0.1, 0.1, units).astype(np.float32)
    fan = units
    for k, u in enumerate(out_units):
        params["output_mlp/%d/kernel" % k] = glorot(rng, fan, u)
        params["output_mlp/%d/bias" % k] = rng.uniform(-0.1, 0.1, u).astype(np.float32)
        fan = u
    return {"attrs": rng.normal(size=(n, feats)).astype(np.float32), "idx": idx, "w": w, "deg": deg, "N": n,
            "ns": np.array([0, n], np.int64), "es": np.array([0, len(recv)], np.int64), "params": params,
            "feats": feats, "units": units, "out_units": tuple(out_units)}


def gcn_tiles(deg):
    """The tile starts ``FusedGcn._balanced_tiles`` builds (None when the busiest uniform tile of 16 nodes holds at most
    512 edges): at most 16 consecutive nodes and - unless one node has more - at most ``GCN_TILE_EDGES`` edges a tile."""
    deg = np.asarray(deg)
    n = len(deg)
    ptr = np.concatenate([[0], np.cumsum(deg)])
    uniform = np.diff(ptr[np.minimum(np.arange(0, n + 16, 16), n)])
    if int(uniform.max()) <= 2 * GCN_TILE_EDGES:
        return None
    starts, nodes, edges = [0], 0, 0
    for i in range(n):
        if nodes == 16 or (nodes > 0 and edges + int(deg[i]) > GCN_TILE_EDGES):
            starts.append(i)
            nodes, edges = 0, 0
        nodes += 1
        edges += int(deg[i])
    starts.append(n)
    return np.asarray(starts)


def gcn_windows(deg, units):
    """Largest number of edge windows a tile of the aggregate launch walks."""
    deg = np.asarray(deg)
    starts = gcn_tiles(deg)
    if starts is None:
        starts = np.minimum(np.arange(0, len(deg) + 16, 16), len(deg))
    ptr = np.concatenate([[0], np.cumsum(deg)])
    return int(max(-(-int(e) // GCN_ECAP[units]) for e in np.diff(ptr[starts])))
