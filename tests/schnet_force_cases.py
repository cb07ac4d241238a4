"""Cases off the molecular shapes for the kernels of the fused SchNet energy + force pass (csrc/mp_schnet_bwd.hip:
``mp_schnet_force_launch``), kernel by kernel, and one composed batch.

``tests/test_gpu_schnet_bwd.py`` and ``tests/test_gpu_forces.py`` run these kernels on QM9- and MD17-shaped molecules
only.  The kernels branch on the basis size (``(bins + 2) >> 1 > 16`` selects the FP32-MFMA build of the distance
gradient), on the edge count against the 32-edge tile, the 128-edge workgroup and the 256-workgroup grid, on a node's
degree against the 64 lanes of the force kernel, on the node count against its 8192 waves and against the 512 persistent
16-node tiles of the node chains, and on a graph's row count against the 8-row rounds and the 24-row prefetch of the
readout.  This module holds seeded generators that reach those branches and one NumPy restatement per operation,
parameterised by dtype (float32 and float64), written from the formulas in the kernel headers - without any engine import:
tests/test_schnet_force_cases.py checks on the CPU that every generator delivers the boundary it claims and that each
float32 restatement is inside half the bar tests/test_gpu_schnet_force_edges.py applies."""
import numpy as np

import topologies as T

F = 128                      # node and filter width
H = 64                       # width of last_mlp's output and of the readout
# csrc/mp_cfconv_bwd.hip
EDGE_TILE = 32               # edges per wave tile (TE)
EDGE_WORKGROUP = 4 * 32      # four waves per workgroup
EDGE_GRID = 256              # workgroups at most: beyond EDGE_TRIP edges the persistent tile loop takes a second trip
EDGE_TRIP = EDGE_GRID * EDGE_WORKGROUP
G1B_MAX_NK = 16              # k pairs the bf16 build of the basis GEMMs holds
MAX_BINS = 32
# csrc/mp_schnet_bwd.hip: schnet_force_kernel
FORCE_LANES = 64             # edges of a node's list per round
FORCE_WAVES = 2048 * 4       # mp::grid_for: 2048 blocks of four waves, one wave per node
# csrc/mp_schnet_node.hip
NODE_TILE = 16
NODE_GRID = 512              # persistent workgroups of the node chains
READOUT_WAVES = 1024 * 4     # one wave per graph
READOUT_ROUND = 8
READOUT_PREFETCH = 24

BAR_CHAIN = 2e-5             # tests/test_gpu_schnet_bwd.py::_close: k-ordered fma chains of length <= 128
BAR_FORCE = 1e-5             # tests/test_gpu_schnet_bwd.py::test_force_from_distance_gradient_over_both_csrs


def fp32_basis_build(bins):
    """True where mp_cfconv_gauss_dist_grad_f32 launches cfconv_dist_grad_kernel<false> (the FP32-MFMA basis GEMMs)."""
    return ((bins + 2) >> 1) > G1B_MAX_NK


def max_rel(got, want):
    """``_close`` of tests/test_gpu_schnet_bwd.py as a number: largest error over the tensor's largest magnitude."""
    want = np.asarray(want, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - want))) / max(float(np.max(np.abs(want))), 1e-6)


def _f32(x):
    return np.float32(x)


def _sigmoid(x):
    t = x.dtype.type
    with np.errstate(over="ignore"):
        return (t(1) / (t(1) + np.exp(-x))).astype(x.dtype)


def _ssp(x):
    t = x.dtype.type
    return (np.logaddexp(t(0), x) - np.log(t(2))).astype(x.dtype)


def _as(a, dtype):
    return None if a is None else np.asarray(a).astype(dtype)


# ------------------------------------------------------------------------------------- A. distance gradient of cfconv
DIST_GRAD_BASE = dict(bins=20, distance=5.0, sigma=0.4, offset=0.0)
SMALL_NODES, SMALL_EDGES = 40, 1300
SATURATED_PRE = 100.0
OOB_EDGES = {3: (-1, None), 40: (None, -1), 700: ("N", None), 1299: (None, "N"), 64: (-1, "N")}   # edge -> (recv, send)


def dist_grad_cases():
    """name -> keyword arguments of ``dist_grad_case``."""
    out = {}
    for bins in (1, 2, 30, 31, 32):
        out["bins%d" % bins] = dict(graph="small", bins=bins)
    out["bins32-nobias"] = dict(graph="small", bins=32, bias=False)
    out["bins20-nobias"] = dict(graph="small", bins=20, bias=False)
    for m in (1, 31, 32, 33, 127, 128, 129):
        out["exact%d" % m] = dict(graph="exact%d" % m)
    out["trip-bins20"] = dict(graph="many%d" % (EDGE_TRIP + 33), bins=20)
    out["trip-bins32"] = dict(graph="many%d" % (EDGE_TRIP + 33), bins=32)
    out["nine-workgroups"] = dict(graph="many%d" % (9 * EDGE_WORKGROUP))
    for kind in ("sorted", "shuffled", "selfdup"):      # 260 points spread over 2.5 A: the basis reaches 8 A
        out["hub-" + kind] = dict(graph="hub-" + kind, distance=8.0)
    out["d-zero"] = dict(graph="small", special="zero")
    out["d-far"] = dict(graph="small", special="far")
    out["offset"] = dict(graph="small", offset=0.75)
    out["sigma0.1"] = dict(graph="small", sigma=0.1)
    out["saturated"] = dict(graph="small", special="saturated")
    out["accumulate"] = dict(graph="small", seed=5)
    out["clamped-indices"] = dict(graph="small", special="oob")
    return out


def _random_pairs(rng, n, m):
    recv = np.sort(rng.integers(0, n, size=m))
    send = (recv + rng.integers(1, n, size=m)) % n
    return np.stack([recv, send], axis=-1).astype(np.int64)


def _edge_graph(graph, rng, seed):
    """(n, edges (M, 2) [receiver, sender], xyz (n, 3) float64)."""
    if graph == "small":
        return SMALL_NODES, _random_pairs(rng, SMALL_NODES, SMALL_EDGES), T.points(rng, SMALL_NODES, 1.2)
    if graph.startswith("exact"):
        n, e = T.tile_exact(int(graph[5:]), n=5, seed=seed)
        return n, e, T.points(rng, n, 1.2)
    if graph.startswith("many"):
        return SMALL_NODES, _random_pairs(rng, SMALL_NODES, int(graph[4:])), T.points(rng, SMALL_NODES, 1.2)
    if graph.startswith("hub"):
        selfdup = graph == "hub-selfdup"
        e = T.hub_edges(260, T.STANDARD_DEGREES, seed, self_loops=selfdup, duplicates=selfdup,
                        order="shuffled" if graph == "hub-shuffled" else "sorted")
        return 260, e, T.points(rng, 260, 2.5, min_distance=0.5)
    raise KeyError(graph)


def dist_grad_case(graph="small", bins=20, distance=5.0, sigma=0.4, offset=0.0, bias=True, special=None, seed=0):
    """Operands of one mp_cfconv_bwd_pack_f32 + mp_cfconv_gauss_dist_grad_f32 call: ``x`` and ``g_out`` (N, 128), the
    distances of the edges between seeded points (float32), ``W1`` (bins, 128) and ``b1`` of the filter's first layer,
    ``W2`` (128, 128).  ``distance``, ``sigma`` and ``offset`` are rounded to float32 (what the C ABI takes), so both
    precisions of the restatement and the kernel read the same numbers.  ``special``: "zero" / "far" put d = 0 / d = 3 x
    ``distance`` on eight edges, "saturated" scales W1 until the largest |pre1| is ``SATURATED_PRE``, "oob" writes the out-of-range node ids of ``OOB_EDGES`` (the kernel clamps them)."""
    rng = np.random.default_rng(7000 + 131 * seed + bins)
    n, e, xyz = _edge_graph(graph, rng, seed)
    m = len(e)
    recv, send = e[:, 0].astype(np.int32), e[:, 1].astype(np.int32)
    dist = np.linalg.norm(xyz[recv] - xyz[send], axis=1).astype(np.float32) if m else np.zeros(0, np.float32)
    c = {"N": n, "M": m, "bins": bins, "distance": float(_f32(distance)), "sigma": float(_f32(sigma)),
         "offset": float(_f32(offset)), "special": special,
         "w1": (rng.standard_normal((bins, F)) * 0.3).astype(np.float32),
         "b1": (rng.standard_normal(F) * 0.1).astype(np.float32) if bias else None,
         "w2": (rng.standard_normal((F, F)) * 0.1).astype(np.float32),
         "x": rng.standard_normal((n, F)).astype(np.float32), "g_out": rng.standard_normal((n, F)).astype(np.float32)}
    c["marked"] = np.zeros(0, np.int64)
    if special in ("zero", "far"):
        c["marked"] = np.sort(rng.choice(m, size=8, replace=False))
        dist[c["marked"]] = 0.0 if special == "zero" else 3.0 * c["distance"]
    elif special == "oob":
        c["marked"] = np.array(sorted(OOB_EDGES), np.int64)
        for edge, (r, s) in OOB_EDGES.items():
            if r is not None:
                recv[edge] = n if r == "N" else r
            if s is not None:
                send[edge] = n if s == "N" else s
    c.update(recv=recv, send=send, dist=dist)
    if special == "saturated":
        for _ in range(3):                      # (the bias is not scaled: the span is reached by iterating)
            c["w1"] *= np.float32(SATURATED_PRE / np.abs(pre1_of(c)).max())
    return c


def _basis(c, dtype):
    """Gauss basis (M, bins) of the case's distances and its derivative w.r.t. the distance (kgcnn/layers/geom.py:554-571:
    centres k / bins * distance, gamma = 1 / (2 sigma^2))."""
    t = np.dtype(dtype).type
    mu = np.arange(c["bins"]).astype(dtype) / t(c["bins"]) * t(c["distance"])
    gamma = t(1.0 / c["sigma"] / c["sigma"] / 2.0)
    v = (c["dist"].astype(dtype)[:, None] - t(c["offset"])) - mu[None, :]
    gauss = np.exp(-gamma * v * v)
    return gauss.astype(dtype), (gauss * (t(-2) * gamma * v)).astype(dtype)


def pre1_of(c, dtype=np.float64):
    gauss, _ = _basis(c, dtype)
    pre = gauss @ c["w1"].astype(dtype)
    return pre + c["b1"].astype(dtype) if c["b1"] is not None else pre


def dist_grad_restate(c, dtype):
    """``g_d[e] = sum_f g_out[recv(e), f] x[send(e), f] dw_f/dd`` with ``w = ssp(gauss(d) W1 + b1) W2 + b2``:
    ``dw/dd = ((gauss'(d) W1) * sigmoid(pre1)) W2``.  Node ids outside ``[0, N)`` are clamped, as the kernel does."""
    if c["M"] == 0:
        return np.zeros(0, dtype)
    _, dgauss = _basis(c, dtype)
    sig = _sigmoid(pre1_of(c, dtype))
    dw = ((dgauss @ c["w1"].astype(dtype)) * sig) @ c["w2"].astype(dtype)
    recv, send = np.clip(c["recv"], 0, c["N"] - 1), np.clip(c["send"], 0, c["N"] - 1)
    return np.sum(c["g_out"][recv].astype(dtype) * c["x"][send].astype(dtype) * dw, axis=1, dtype=dtype)


# ------------------------------------------------------------------------------------- B. forces from dE/dd
RING_NODES = FORCE_WAVES + 17
RING_STEP = 3


def force_cases():
    return {"receiver-hubs": dict(graph="hub"), "sender-hubs": dict(graph="hub-swapped"),
            "shuffled-hubs": dict(graph="hub-shuffled"), "hubs-selfdup-plus": dict(graph="hub-selfdup", scale=1.0),
            "node-trip": dict(graph="ring"), "no-edges": dict(graph="empty")}


def force_case(graph="hub", scale=-1.0, seed=0):
    """Operands of one mp_schnet_force_from_gd_f32 call: one graph of ``N`` points, ``edges`` (M, 2) local = global
    ``[receiver, sender]``, float32 distances of the float32 coordinates, a random ``g_d`` (M).  Two pairs of distinct
    nodes are moved onto each other (d = 0: they contribute nothing); self loops have d = 0 as well."""
    rng = np.random.default_rng(8000 + seed)
    if graph == "ring":
        n, e = RING_NODES, T.ring_edges(RING_NODES, RING_STEP)
        xyz = rng.normal(0.0, 6.0, size=(n, 3))
    elif graph == "empty":
        n, e, xyz = 37, np.zeros((0, 2), np.int64), rng.normal(0.0, 2.0, size=(37, 3))
    else:
        n = 260
        selfdup = graph == "hub-selfdup"
        e = T.hub_edges(n, T.STANDARD_DEGREES, seed + 4, self_loops=selfdup, duplicates=selfdup,
                        order="shuffled" if graph == "hub-shuffled" else "sorted")
        if graph == "hub-swapped":
            e = T.swap_columns(e)
        xyz = T.points(rng, n, 2.5, min_distance=0.5)
    xyz = xyz.astype(np.float32)
    coincident = np.zeros(0, np.int64)
    if len(e):
        apart = np.nonzero(e[:, 0] != e[:, 1])[0]
        first = apart[len(apart) // 3]
        free = apart[~np.isin(e[apart], e[first]).any(axis=1)]          # pairs that share no node with the first
        coincident = np.array([first, free[(2 * len(free)) // 3]], np.int64)
        for k in coincident:
            xyz[e[k, 1]] = xyz[e[k, 0]]
    diff = xyz[e[:, 0]].astype(np.float64) - xyz[e[:, 1]].astype(np.float64)
    dist = np.linalg.norm(diff, axis=1).astype(np.float32)
    return {"N": n, "M": len(e), "edges": e, "recv": e[:, 0].astype(np.int32), "send": e[:, 1].astype(np.int32),
            "xyz": xyz, "dist": dist, "g_d": rng.standard_normal(len(e)).astype(np.float32), "scale": float(scale),
            "coincident": coincident}


def force_restate(c, dtype):
    """``F_n = scale * sum_e g_d[e] (x_n - x_other) / d_e`` over the edges that hold ``n`` in either column, nothing
    from an edge with ``d == 0`` (divide_no_nan)."""
    out = np.zeros((c["N"], 3), dtype)
    keep = c["dist"] != 0
    recv, send = c["recv"][keep], c["send"][keep]
    xyz = c["xyz"].astype(dtype)
    t = (c["g_d"][keep].astype(dtype) / c["dist"][keep].astype(dtype))[:, None] * (xyz[recv] - xyz[send])
    np.add.at(out, recv, t)
    np.add.at(out, send, -t)
    return (np.dtype(dtype).type(c["scale"]) * out).astype(dtype)


# ------------------------------------------------------------------------------------- C. SAVE builds of the node chains
NODE_COUNTS = (1, 15, 16, 17, NODE_GRID * NODE_TILE + 1)
TAIL_ROWS = 3                # sentinel rows behind the N rows of every node buffer
SATURATED_SPAN = 30.0


def node_case(n, bias=True, saturated=False, seed=0):
    """Operands of the MID and the LAST chain on ``n`` nodes: aggregated messages ``agg`` and node state ``n`` (N, 128),
    kernels in N(0, 0.1^2) and biases in +-0.1 (``bias=False``: every bias absent).  ``saturated``: ``agg`` and
    ``Wl0`` are scaled until the largest |agg W2 + b2| and |n' Wl0 + bl0| are ``SATURATED_SPAN``."""
    rng = np.random.default_rng(9000 + 17 * seed + n)
    w = lambda k, u: (rng.standard_normal((k, u)) * 0.1).astype(np.float32)
    b = lambda u: rng.uniform(-0.1, 0.1, size=u).astype(np.float32) if bias else None
    c = {"N": n, "agg": rng.standard_normal((n, F)).astype(np.float32), "n": rng.standard_normal((n, F)).astype(np.float32),
         "W2": w(F, F), "b2": b(F), "W3": w(F, F), "b3": b(F), "Wx": w(F, F), "Wl0": w(F, F), "bl0": b(F),
         "Wl1": w(F, H), "bl1": b(H), "saturated": saturated}
    if saturated:
        pre2 = np.abs(node_restate(c, np.float64)["pre2"]).max()
        c["agg"] *= np.float32(SATURATED_SPAN / pre2)
        for _ in range(3):                      # (the bias is not scaled: the span is reached by iterating)
            c["Wl0"] *= np.float32(SATURATED_SPAN / np.abs(node_restate(c, np.float64)["prel0"]).max())
    return c


def node_restate(c, dtype):
    """MID: ``t = ssp(agg W2 + b2); n' = n + t W3 + b3; x = n' Wx`` with ``d2 = sigmoid(agg W2 + b2)``;
    LAST: the same ``n'``, then ``u = ssp(n' Wl0 + bl0); h = ssp(u Wl1 + bl1)`` with ``dl0``, ``dl1`` the sigmoids of the
    two pre-activations."""
    f = lambda k: _as(c[k], dtype)
    add = lambda y, bias: y if bias is None else y + bias
    pre2 = add(f("agg") @ f("W2"), f("b2"))
    n_new = f("n") + add(_ssp(pre2) @ f("W3"), f("b3"))
    prel0 = add(n_new @ f("Wl0"), f("bl0"))
    prel1 = add(_ssp(prel0) @ f("Wl1"), f("bl1"))
    return {"pre2": pre2, "prel0": prel0, "prel1": prel1, "d2": _sigmoid(pre2), "n": n_new, "x": n_new @ f("Wx"),
            "dl0": _sigmoid(prel0), "dl1": _sigmoid(prel1), "h": _ssp(prel1)}


MID_OUTPUTS = ("n", "x", "d2")
LAST_OUTPUTS = ("h", "d2", "dl0", "dl1")


# ------------------------------------------------------------------------------------- D. readout and dE/dpooled
READOUT_SIZES = (0, 1, 7, 8, 9, 23, 24, 25, 33, 100, 0, 16, 0)
READOUT_TRIP_GRAPHS = READOUT_WAVES + 5


def readout_case(sizes=READOUT_SIZES, bias=(True, True), seed=0):
    """Rows ``h`` (N, 64) in 0..0.1 over graphs of ``sizes`` rows, ``Wo0`` (64, 64) Glorot, ``Wo1`` (64, 1) in 0.05..0.3,
    ``bo0`` in 0.2..0.5 and ``bo1`` in 0.05..0.1 (``bias`` switches either off).  An energy is one number per graph: with
    signed ``Wo1`` or a ``bo0`` around 0 the graphs of 0 to 2 rows have energies that cancel to 1e-4 of the batch's
    largest, where the 1e-3 floor of ``parity.rowwise_rel`` reads float32 rounding as 3e-4."""
    rng = np.random.default_rng(9500 + seed)
    sizes = np.asarray(sizes, np.int64)
    n = int(sizes.sum())
    lim = np.sqrt(6.0 / (H + H))
    return {"sizes": sizes, "splits": np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), "G": len(sizes), "N": n,
            "h": rng.uniform(0.0, 0.1, size=(n, H)).astype(np.float32),
            "Wo0": rng.uniform(-lim, lim, size=(H, H)).astype(np.float32),
            "bo0": rng.uniform(0.2, 0.5, size=H).astype(np.float32) if bias[0] else None,
            "Wo1": rng.uniform(0.05, 0.3, size=(H, 1)).astype(np.float32),
            "bo1": rng.uniform(0.05, 0.1, size=1).astype(np.float32) if bias[1] else None}


def readout_trip_sizes(seed=0):
    return np.random.default_rng(9600 + seed).integers(0, 3, size=READOUT_TRIP_GRAPHS)


def readout_restate(c, dtype, head="mlp"):
    """(out (G, 1), g_pool (G, 64) or None).  "mlp": ``pooled = sum of the graph's rows; out = ssp(pooled Wo0 + bo0) Wo1 +
    bo1`` and ``dE/dpooled = Wo0 (Wo1 * sigmoid(pooled Wo0 + bo0))``; "linear" (no Wo0): ``out = sum_n h_n . Wo1 + n_g bo1``."""
    h = c["h"].astype(dtype)
    pooled = np.zeros((c["G"], H), dtype)
    np.add.at(pooled, np.repeat(np.arange(c["G"]), c["sizes"]), h)
    w1 = c["Wo1"].astype(dtype)
    b1 = np.zeros(1, dtype) if c["bo1"] is None else c["bo1"].astype(dtype)
    if head == "linear":
        return (pooled @ w1 + c["sizes"].astype(dtype)[:, None] * b1[None, :]).astype(dtype), None
    pre = pooled @ c["Wo0"].astype(dtype)
    if c["bo0"] is not None:
        pre = pre + c["bo0"].astype(dtype)
    out = _ssp(pre) @ w1 + b1[None, :]
    return out.astype(dtype), ((_sigmoid(pre) * w1[:, 0][None, :]) @ c["Wo0"].astype(dtype).T).astype(dtype)


# ------------------------------------------------------------------------------------- E. composed batch
# the recipe of topologies.EGNN_MODEL_BATCH: a compact 70-atom molecule whose atoms all have more than 64 neighbours inside
# 8 A, a lone atom, an empty graph and an aspirin-sized molecule
MODEL_BATCH = dict(sizes=(70, 1, 0, 21), seed=22, min_distance=0.9, max_distance=8.0, sigma=1.2)
MODEL_GAUSS = {32: {"bins": 32, "distance": 8, "offset": 0.0, "sigma": 0.4},
               25: {"bins": 25, "distance": 8, "offset": 0.0, "sigma": 0.4}}
ASPIRIN_Z = np.array([6] * 9 + [1] * 8 + [8] * 4, dtype=np.float32)


def model_batch(radius_graph, shuffled=False):
    """Flat batch (node_number, node_coordinates, edge_indices, node_splits, edge_splits) of ``MODEL_BATCH``;
    ``radius_graph`` is ``gcnn_keras_amd.synth.radius_graph`` (handed in: this module imports no package code), called
    with ``max_neighbours=None``.  ``shuffled``: the edges of every graph in random order."""
    spec = MODEL_BATCH
    rng = np.random.default_rng(spec["seed"])
    xs = [T.points(rng, n, spec["sigma"], spec["min_distance"]).reshape(n, 3) for n in spec["sizes"]]
    es = [radius_graph(x, max_distance=spec["max_distance"], max_neighbours=None).reshape(-1, 2) if len(x) else
          np.zeros((0, 2), np.int64) for x in xs]
    if shuffled:
        es = [e[rng.permutation(len(e))] for e in es]
    splits = lambda lens: np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return {"node_number": np.concatenate([np.resize(ASPIRIN_Z, n) for n in spec["sizes"]]).astype(np.float32),
            "node_coordinates": np.concatenate(xs, axis=0).astype(np.float32).reshape(-1, 3),
            "edge_indices": np.concatenate(es, axis=0).reshape(-1, 2).astype(np.int64),
            "node_splits": splits(spec["sizes"]), "edge_splits": splits([len(e) for e in es])}
