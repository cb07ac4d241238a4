"""Cases off the molecular shapes for the fused continuous-filter convolution (csrc/mp_cfconv.hip: ``cfconv_fused_kernel``,
``cfconv_pack_kernel``, ``cfconv_boundary_kernel``), and its NumPy restatement.

``tests/test_gpu_fused.py`` runs the kernel on QM9-shaped batches (in-degree <= 28: a 32-edge tile holds one or two
segments), on one hub graph and at four basis sizes of the Gauss entry point.  The kernel branches on the wave-uniform
shape of a tile's 32-bit start mask (segments touching the low half ``nlo``, the high half ``nhi``, whether edge 16
continues edge 15, whether a half already holds an opened segment when the next one opens), on whether the tile's first
and last segment continue in the neighbouring tiles, on the edge count against tile, workgroup and the 256-workgroup grid,
on the basis size (``nk = (B + 2) >> 1``: fixed builds for 20 and 25, the generic one elsewhere) and on absent biases.
This module holds seeded generators that reach those branches - all built on tests/topologies.py - and one restatement,
parameterised by dtype (float32 and float64), written from the formulas in the kernel header and kgcnn/layers/geom.py,
without any engine import: tests/test_cfconv_cases.py checks on the CPU that every generator delivers the layout it
claims and that the float32 restatement is inside half the bar tests/test_gpu_cfconv_edges.py applies."""
import functools

import numpy as np

import topologies as T

F = 128                      # node and filter width of the fused kernel
TILE = 32                    # edges per wave tile (TE)
MAX_BINS = 32                # MAX_KROWS - 2
G1B_MAX_NK = 16              # k pairs the bf16 image of W1 holds
MAX_KROWS = 34
W2_PIECE_FLOATS = F * F // 2
W1B_FLOATS = 3 * 2 * 4 * 64 * 4
PACKED_FLOATS = MAX_KROWS * F + 3 * W2_PIECE_FLOATS + F + W1B_FLOATS

SATURATED_PRE = 100.0

# ------------------------------------------------------------------------------------------------ A. layout graph
# per-tile degree patterns, each summing to 32: the receivers of a pattern fill exactly one tile
FIXED_PATTERNS = ([[32]] + [[k, 32 - k] for k in range(1, 32)]
                  + [[1] * 32, [2] * 16, [16, 16], [15, 1, 1, 15], [15, 2, 15], [1, 30, 1], [8, 8, 8, 8],
                     [1, 14, 1, 1, 14, 1]])
RANDOM_PATTERNS = 40


def random_compositions(count, seed):
    """``count`` seeded compositions of 32 into 2..12 positive parts."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        parts = int(rng.integers(2, 13))
        cuts = np.sort(rng.choice(np.arange(1, TILE), size=parts - 1, replace=False))
        out.append([int(v) for v in np.diff(np.concatenate([[0], cuts, [TILE]]))])
    return out


def layout_patterns(seed=0):
    return [list(p) for p in FIXED_PATTERNS] + random_compositions(RANDOM_PATTERNS, 100 + seed)


def layout_degrees(seed=0):
    """In-degrees of consecutive receivers: the patterns one after another, 0 to 2 receivers without edges between them
    (and one in front)."""
    rng = np.random.default_rng(200 + seed)
    degrees = [0]
    for p in layout_patterns(seed):
        degrees += p + [0] * int(rng.integers(0, 3))
    return degrees


def _selfdup(e, seed):
    """One self loop and one duplicated sender inside every tile-sized run of ``e`` (sorted by receiver): edge i sends
    to its own receiver; edge j, which shares its receiver with edge j - 1, repeats that edge's sender (skipped in a run
    of single-edge receivers)."""
    rng = np.random.default_rng(300 + seed)
    e = e.copy()
    for lo in range(0, len(e) - TILE + 1, TILE):
        i = lo + int(rng.integers(0, TILE))
        e[i, 1] = e[i, 0]
        pairs = [j for j in range(lo + 1, lo + TILE) if e[j, 0] == e[j - 1, 0] and j != i and j - 1 != i]
        if pairs:
            j = pairs[int(rng.integers(0, len(pairs)))]
            e[j, 1] = e[j - 1, 1]
    return e


def layout_graph(seed=0):
    """(n, edges): case A.  Node 0 and the last node receive nothing."""
    degrees = layout_degrees(seed)
    n = len(degrees) + 1
    return n, _selfdup(T.degree_edges(n, degrees, 400 + seed), seed)


# ------------------------------------------------------------------------------------------------ B. unaligned graph
UNALIGNED_DEGREES = (1, 2, 3, 5, 16, 17, 31, 32, 33, 48, 64, 65, 100)
UNALIGNED_RECEIVERS = 600
UNALIGNED_SEED = 3           # (with 600 receivers most seeds reach every layout class; the CPU test asserts this one does)
WHOLE_TILES_DEGREE = 1000    # 30 or 31 whole tiles, wherever it starts


def unaligned_degrees(seed=0):
    rng = np.random.default_rng(500 + UNALIGNED_SEED + seed)
    deg = [int(v) for v in rng.choice(UNALIGNED_DEGREES, size=UNALIGNED_RECEIVERS)]
    deg.insert(UNALIGNED_RECEIVERS // 2, WHOLE_TILES_DEGREE)
    return deg


def unaligned_graph(seed=0, edges=None):
    """(n, edges): case B; ``edges``: only the first so many edges (the later receivers then receive nothing)."""
    degrees = unaligned_degrees(seed)
    n = len(degrees) + 2
    e = T.degree_edges(n, degrees, 600 + UNALIGNED_SEED + seed, first=1)
    return n, (e if edges is None else e[:edges])


# ------------------------------------------------------------------------------------------------ tile masks
def start_masks(recv_sorted):
    """The kernel's 32-bit start mask of every tile of a receiver-sorted list: bit c (1..31) set where edge c of the tile
    has another receiver than edge c - 1; padding edges of the last tile repeat the last receiver."""
    r = np.asarray(recv_sorted, np.int64)
    tiles = -(-len(r) // TILE)
    r = np.concatenate([r, np.full(tiles * TILE - len(r), r[-1] if len(r) else 0)]).reshape(tiles, TILE)
    bits = np.zeros((tiles, TILE), bool)
    bits[:, 1:] = r[:, 1:] != r[:, :-1]
    return (bits.astype(np.uint64) << np.arange(TILE, dtype=np.uint64)).sum(axis=1).astype(np.uint64)


def tile_shapes(recv_sorted):
    """One dict per tile: the wave-uniform quantities the segment walk branches on (csrc/mp_cfconv.hip) - ``nlo``, ``nhi``,
    ``cont``, the openings inside either half (bits 1..15 / 17..31), and whether the tile's first / last segment
    continues from the previous / into the next tile."""
    r = np.asarray(recv_sorted, np.int64)
    out = []
    for t, sm in enumerate(int(v) for v in start_masks(r)):
        lo, hi = t * TILE, min((t + 1) * TILE, len(r))
        open_lo, open_hi = bin(sm & 0xfffe).count("1"), bin(sm >> 17).count("1")
        out.append({"mask": sm, "nlo": open_lo + 1, "nhi": open_hi + 1, "cont": ((sm >> 16) & 1) == 0,
                    "open_lo": open_lo, "open_hi": open_hi,
                    "from_prev": lo > 0 and r[lo - 1] == r[lo], "into_next": hi < len(r) and r[hi] == r[hi - 1]})
    return out


def shape_class(s):
    return (s["nlo"] > 1, s["cont"], s["nhi"] > 1)


# ------------------------------------------------------------------------------------------------ cases
EXACT_COUNTS = (1, 31, 32, 33, 127, 128, 129, 255, 256, 257)
SWEEP_GROUPS = tuple(range(1, 18))                  # M = 128 g - 5: g workgroups of the 4-wave build
TRIP4_EDGES = TILE * 1024 + 33                      # one tile and one edge past 256 workgroups x 4 waves
TRIP8_EDGES = TILE * 2048 + 33                      # the same for 8 waves
HALF_GRID_EDGES = (257, 1333)
BASES = (1, 2, 19, 20, 21, 24, 25, 26, 30, 31, 32)
TRIMMED_EDGES = 400


def cases():
    """name -> keyword arguments of ``case``."""
    out = {"layout": dict(graph="layout"), "unaligned": dict(graph="unaligned"),
           "layout-shuffled": dict(graph="layout", shuffled=True),
           "unaligned-shuffled": dict(graph="unaligned", shuffled=True)}
    for m in EXACT_COUNTS:
        out["exact%d" % m] = dict(graph="exact%d" % m)
    for g in SWEEP_GROUPS:
        out["sweep%d" % g] = dict(graph="exact%d" % (128 * g - 5))
    # trip8 over 80 nodes, not 40: a float32 sum of 1640 terms in list order is 5.6e-06 from float64 (over the half bar);
    # at 820 terms per receiver, as in trip4, it is 2e-06
    out["trip4"] = dict(graph="many%d" % TRIP4_EDGES)
    out["trip8"] = dict(graph="many%d/80" % TRIP8_EDGES)
    for m in HALF_GRID_EDGES:
        out["half%d" % m] = dict(graph="many%d" % m)
    for b in BASES:
        out["bins%d" % b] = dict(graph="trimmed", bins=b)
    out["no-b1"] = dict(graph="trimmed", bias=(False, True))
    out["no-b2"] = dict(graph="trimmed", bias=(True, False))
    out["no-bias"] = dict(graph="trimmed", bias=(False, False))
    out["offset"] = dict(graph="trimmed", offset=0.75)
    out["sigma0.1-bins32"] = dict(graph="trimmed", sigma=0.1, bins=32)
    out["d-zero"] = dict(graph="trimmed", special="zero")
    out["d-far"] = dict(graph="trimmed", special="far")
    out["saturated"] = dict(graph="trimmed", special="saturated")
    out["layer-det"] = dict(graph="unaligned", shuffled=True, bins=25, bias=(True, True), seed=1)
    out["layer-no-bias"] = dict(graph="trimmed", bias=(False, False), seed=1)
    return out


LAYOUT_CASES = ("layout", "unaligned", "layout-shuffled", "unaligned-shuffled")
COUNT_CASES = tuple("exact%d" % m for m in EXACT_COUNTS) + tuple("sweep%d" % g for g in SWEEP_GROUPS)
TRIP_CASES = ("trip4", "trip8") + tuple("half%d" % m for m in HALF_GRID_EDGES)
BASIS_CASES = tuple("bins%d" % b for b in BASES)
PARAMETER_CASES = ("no-b1", "no-b2", "no-bias", "offset", "sigma0.1-bins32", "d-zero", "d-far", "saturated")
LAYER_CASES = ("layer-det", "layer-no-bias")


def _graph(graph, seed):
    if graph == "layout":
        return layout_graph(seed)
    if graph == "unaligned":
        return unaligned_graph(seed)
    if graph == "trimmed":
        return unaligned_graph(seed, edges=TRIMMED_EDGES)
    if graph.startswith("exact"):
        return T.tile_exact(int(graph[5:]), n=5, seed=seed)
    if graph.startswith("many"):            # "many<M>" over 40 nodes, "many<M>/<n>" over n
        m, _, n = graph[4:].partition("/")
        return T.tile_exact(int(m), n=int(n or 40), seed=seed)
    raise KeyError(graph)


def case(graph="trimmed", bins=20, distance=5.0, sigma=0.4, offset=0.0, bias=(True, True), special=None,
         shuffled=False, seed=0):
    """Operands of one fused cfconv call: ``x`` (N, 128), edges ``recv`` / ``send`` (M) int32 in list order, the float32
    distances of the edges between seeded points (a self loop has d = 0), ``w1`` (bins, 128), ``b1``, ``w2`` (128, 128),
    ``b2`` (``bias`` switches either off).  ``distance``, ``sigma`` and ``offset`` are rounded to float32 (what the C ABI
    takes), so both precisions of the restatement and the kernel read the same numbers.  ``special``: "zero" / "far" put
    d = 0 / d = 3 x ``distance`` on eight edges, "saturated" scales ``w1`` until the largest |pre-activation| of the
    first layer is ``SATURATED_PRE``.  ``shuffled``: the edge list in random order."""
    rng = np.random.default_rng(11000 + 131 * seed + bins)
    n, e = _graph(graph, seed)
    if shuffled:
        e = e[rng.permutation(len(e))]
    m = len(e)
    xyz = T.points(rng, n, 1.2, min_distance=0.3)
    recv, send = e[:, 0].astype(np.int32), e[:, 1].astype(np.int32)
    dist = np.linalg.norm(xyz[recv] - xyz[send], axis=1).astype(np.float32)
    f32 = lambda v: float(np.float32(v))
    c = {"N": n, "M": m, "bins": bins, "distance": f32(distance), "sigma": f32(sigma), "offset": f32(offset),
         "special": special, "shuffled": shuffled,
         "w1": (rng.standard_normal((bins, F)) * 0.3).astype(np.float32),
         "b1": (rng.standard_normal(F) * 0.1).astype(np.float32) if bias[0] else None,
         "w2": (rng.standard_normal((F, F)) * 0.1).astype(np.float32),
         "b2": (rng.standard_normal(F) * 0.1).astype(np.float32) if bias[1] else None,
         "x": rng.standard_normal((n, F)).astype(np.float32), "marked": np.zeros(0, np.int64)}
    if special in ("zero", "far"):
        c["marked"] = np.sort(rng.choice(m, size=8, replace=False))
        dist[c["marked"]] = 0.0 if special == "zero" else 3.0 * c["distance"]
    c.update(recv=recv, send=send, dist=dist)
    if special == "saturated":
        for _ in range(3):                      # (the bias is not scaled: the span is reached by iterating)
            c["w1"] *= np.float32(SATURATED_PRE / np.abs(pre1_of(c)).max())
    return c


@functools.lru_cache(maxsize=None)
def get(name):
    """The case of that name, built once per process (read-only: tests share it)."""
    c = case(**cases()[name])
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def kernel_order(c):
    """(recv_sorted (M) int32, perm (M) int32 or None): what the kernel takes - the receivers ascending and, unless the
    list is sorted already, the stable permutation sorted position -> list position."""
    if np.all(np.diff(c["recv"]) >= 0):
        return c["recv"], None
    perm = np.argsort(c["recv"], kind="stable").astype(np.int32)
    return np.ascontiguousarray(c["recv"][perm]), perm


# ------------------------------------------------------------------------------------------------ restatement
def _ssp(x):
    t = x.dtype.type
    return (np.logaddexp(t(0), x) - np.log(t(2))).astype(x.dtype)


def gauss_rbf(c, dtype):
    """Gauss basis (M, bins) of the case's distances (kgcnn/layers/geom.py:554-571): centres k / bins * distance,
    gamma = 1 / (2 sigma^2)."""
    t = np.dtype(dtype).type
    mu = np.arange(c["bins"]).astype(dtype) / t(c["bins"]) * t(c["distance"])
    gamma = t(1.0 / c["sigma"] / c["sigma"] / 2.0)
    v = (c["dist"].astype(dtype)[:, None] - t(c["offset"])) - mu[None, :]
    return np.exp(-gamma * v * v).astype(dtype)


def given_rbf(c):
    """The (M, bins) float32 matrix handed to the entry points that take a basis: the Gauss basis, rounded once."""
    return gauss_rbf(c, np.float64).astype(np.float32)


def pre1_of(c, dtype=np.float64, rbf=None):
    rbf = gauss_rbf(c, dtype) if rbf is None else np.asarray(rbf).astype(dtype)
    pre = rbf @ c["w1"].astype(dtype)
    return pre + c["b1"].astype(dtype) if c["b1"] is not None else pre


def cfconv_restate(c, dtype, rbf=None):
    """``out[r] = sum over the edges of receiver r, in list order, of x[send] * (ssp(rbf W1 + b1) W2 + b2)`` (N, 128);
    ``rbf``: a given (M, bins) matrix instead of the Gauss basis of the case's distances."""
    filt = _ssp(pre1_of(c, dtype, rbf)) @ c["w2"].astype(dtype)
    if c["b2"] is not None:
        filt = filt + c["b2"].astype(dtype)
    out = np.zeros((c["N"], F), dtype)
    np.add.at(out, c["recv"], (c["x"].astype(dtype)[c["send"]] * filt).astype(dtype))
    return out


@functools.lru_cache(maxsize=None)
def restated(name, entry="gauss"):
    """(float32, float64) restatements of a named case, computed once: ``entry`` "gauss" (from the distances) or "rbf"
    (from ``given_rbf``)."""
    c = get(name)
    rbf = given_rbf(c) if entry == "rbf" else None
    pair = tuple(cfconv_restate(c, dt, rbf) for dt in (np.float32, np.float64))
    for a in pair:
        a.setflags(write=False)
    return pair


# ------------------------------------------------------------------------------------------------ pack image
def rowmap(r, hh):
    return (r & 3) + 8 * (r >> 2) + 4 * hh


def bf16_to_float64(u16):
    return (np.asarray(u16, np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def decode_w2_images(image_floats):
    """(3, 128, 128) float64: the hi, mid and lo bf16 images of W2, from the layout in the kernel's comments - 16 B per
    (piece, k block m, column block jb, lane): element i = piece(W2[f][4 c + jb]), f = 32 (m >> 1) + rowmap(8 (m & 1) + i,
    hh), c = lane & 31, hh = lane >> 5."""
    u = np.ascontiguousarray(image_floats, np.float32).view(np.uint16).reshape(3, 8, 4, 64, 8)
    out = np.full((3, F, F), np.nan)
    for m in range(8):
        for jb in range(4):
            for lane in range(64):
                c, hh = lane & 31, lane >> 5
                for i in range(8):
                    f = 32 * (m >> 1) + rowmap(8 * (m & 1) + i, hh)
                    out[:, f, 4 * c + jb] = bf16_to_float64(u[:, m, jb, lane, i])
    return out


def decode_w1_images(image_floats, bins):
    """(3, 34, 128) float64: the bf16 images of W1 | b1 | zero rows - 16 B per (piece, k block kb, hidden block ib, lane):
    element i = piece(W1ext[k][32 ib + c]), s = 8 kb + i, k = s + nk hh for s < nk - and the largest magnitude in the
    slots s >= nk (which hold zeros)."""
    nk = (bins + 2) >> 1
    u = np.ascontiguousarray(image_floats, np.float32).view(np.uint16).reshape(3, 2, 4, 64, 8)
    out = np.zeros((3, MAX_KROWS, F))
    unused = 0.0
    for kb in range(2):
        for ib in range(4):
            for lane in range(64):
                c, hh = lane & 31, lane >> 5
                for i in range(8):
                    s = 8 * kb + i
                    v = bf16_to_float64(u[:, kb, ib, lane, i])
                    if s < nk:
                        out[:, s + nk * hh, 32 * ib + c] = v
                    else:
                        unused = max(unused, float(np.abs(v).max()))
    return out, unused
