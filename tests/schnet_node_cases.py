"""Cases for the inference builds of the SchNet node chains (csrc/mp_schnet_node.hip), kernel by kernel: the MID and LAST
chains on FP32 matrix instructions and as bf16 pieces, on the full and on the half grid; the input chain
``Dense(Embedding(z))``; stage 0 (input chain + edge preparation in one launch) on both sides of its fallback thresholds;
the layer-path build on raw Keras kernels; the two weight packers.

``launch_node_impl`` keeps at most 512 (FP32), 256 (bf16 pieces) or, with flag bit 9 from 256 tiles on, 128 persistent
workgroups of one 16-node tile each; ``mp_schnet_stage0_f32`` runs both roles in one launch up to 1024 tiles and 1023
graphs.  The constants below restate those caps, the node counts are derived from them, and tests/test_schnet_node_cases.py
asserts on the CPU which situation every count produces (tiles, tiles per workgroup, rows of the last tile).

This module holds seeded generators and NumPy restatements parameterised by dtype, written from the formulas in the
kernel's header and in the comments above the pack kernels - without any engine import.  The MID / LAST operands and their
restatement are those of the SAVE-build test (``node_case`` / ``node_restate`` of tests/schnet_force_cases.py), imported,
not copied.  tests/test_gpu_schnet_node_edges.py holds every floating-point comparison to ``BAR_CHAIN``."""
import numpy as np
import torch

from schnet_force_cases import BAR_CHAIN, F, H, max_rel, node_case, node_restate   # noqa: F401 (re-exported)

# ---------------------------------------------------------------------------------- launch_node_impl, flag bits
TILE = 16                    # nodes per tile (RB = 1)
CAP_FP32 = 512               # persistent workgroups of the FP32 builds
CAP_BF = 256                 # of the bf16-piece builds
CAP_BF_HALF = 128            # of the bf16-piece builds with flag bit 9 ...
HALF_FROM_TILES = 256        # ... from this many tiles on
FAST, PACKED, BF, I64, HALF = 1, 2, 64, 256, 512          # flag bits 0, 1, 6, 8, 9

CHAIN_FLAGS = (PACKED, PACKED | FAST, PACKED | BF, PACKED | FAST | BF, PACKED | BF | HALF, PACKED | FAST | BF | HALF)
EDGE_COUNTS = (1, TILE - 1, TILE, TILE + 1)
TRIP_FP32 = CAP_FP32 * TILE + 1                 # one workgroup of the FP32 builds takes a second tile, of one row
TRIP_BF = CAP_BF * TILE + 1                     # the same for the bf16-piece builds
HALF_FULL = (HALF_FROM_TILES - 1) * TILE        # 255 tiles: bit 9 does not apply yet
HALF_TWO = (HALF_FROM_TILES - 1) * TILE + 1     # 256 tiles on 128 workgroups: two each, the last of one row
HALF_THREE = HALF_FROM_TILES * TILE + 1         # 257 tiles: workgroup 0 takes three
SATURATED_N = 37


def tiles(n):
    return -(-n // TILE)


def cap_of(flags, n):
    """``cap`` of launch_node_impl (and ``node_cap`` of mp_schnet_stage0_f32)."""
    if not flags & BF:
        return CAP_FP32
    return CAP_BF_HALF if (flags & HALF) and tiles(n) >= HALF_FROM_TILES else CAP_BF


def grid_of(flags, n):
    return min(tiles(n), cap_of(flags, n))


def tiles_per_workgroup(flags, n):
    """(fewest, most) tiles a workgroup of the launch takes: workgroup b takes tiles b, b + grid, ..."""
    t, g = tiles(n), grid_of(flags, n)
    return t // g, -(-t // g)


def last_tile_rows(n):
    return n - (tiles(n) - 1) * TILE


def trip_counts(flags):
    """Node counts past the persistent grid of the family ``flags`` selects."""
    if not flags & BF:
        return (TRIP_FP32,)
    return (HALF_FULL, HALF_TWO, HALF_THREE) if flags & HALF else (TRIP_BF,)


def chain_counts(flags):
    return EDGE_COUNTS + trip_counts(flags)


def chain_runs(flags):
    """(n, bias, saturated) of every MID / LAST run of one flag set: the tile edges and the trips with biases, every bias
    absent at 17 nodes and on the family's trips (with bit 9: two and three tiles per workgroup), one saturated case."""
    nobias = (TILE + 1,) + tuple(n for n in trip_counts(flags) if n != HALF_FULL)
    return [(n, True, False) for n in chain_counts(flags)] + [(n, False, False) for n in nobias] + \
        [(SATURATED_N, True, True)]


# ---------------------------------------------------------------------------------- B. input chain
VOCAB = 95
IN_FLAGS = (PACKED, PACKED | FAST, PACKED | BF, PACKED | FAST | BF, PACKED | FAST | BF | HALF)
IN_PATTERNS = ("uniform", "same", "ends", "oob", "fractional", "oob-last", "oob-first")
OOB_NUMBERS = (-1, "vocab", 1000)
OOB_NUMBERS_I64 = (-1, "vocab", 1000, 2 ** 31 + 3)        # the last one wraps to a negative int32
FRACTIONS = (5.7, 94.5, -0.5)                             # truncate to 5, 94 and 0: all valid rows of the default vocabulary


def in_counts(flags):
    extra = (TRIP_FP32,) if not flags & BF else ((TRIP_BF, HALF_TWO) if flags & HALF else (TRIP_BF,))
    return EDGE_COUNTS + (2 * TILE + 1,) + extra


def in_runs(flags, i64):
    """(n, pattern, vocab) of every input-chain run of one build: uniform numbers at every count; every pattern at 17 and
    33 nodes; an out-of-range number on the one row of the trip's last tile, on the last row of a full tile, on row 0 of a
    one-node and of a 16-node batch; a vocabulary of 1."""
    patterns = [p for p in IN_PATTERNS if not (i64 and p == "fractional")]
    runs = [(n, "uniform", VOCAB) for n in in_counts(flags)]
    runs += [(n, p, VOCAB) for n in (TILE + 1, 2 * TILE + 1) for p in patterns if p != "uniform"]
    runs += [(n, "oob-last", VOCAB) for n in in_counts(flags)[-2:] + (TILE,)]
    runs += [(1, "oob-first", VOCAB), (TILE, "oob-first", VOCAB), (in_counts(flags)[-1], "oob", VOCAB)]
    runs += [(TILE + 1, "uniform", 1), (TILE + 1, "oob", 1), (2 * TILE + 1, "oob-last", 1)]
    return list(dict.fromkeys(runs))


def in_weights(emb_dim, vocab=VOCAB, seed=0):
    """Embedding (vocab, emb_dim) in N(0, 1), ``W0`` (emb_dim, 128) and ``Wx`` (128, 128) in N(0, 0.1^2), ``b0`` in +-0.1."""
    rng = np.random.default_rng(9700 + 13 * seed + emb_dim + 1000 * vocab)
    return {"vocab": vocab, "emb_dim": emb_dim, "emb": rng.standard_normal((vocab, emb_dim)).astype(np.float32),
            "W0": (rng.standard_normal((emb_dim, F)) * 0.1).astype(np.float32),
            "b0": rng.uniform(-0.1, 0.1, size=F).astype(np.float32),
            "Wx": (rng.standard_normal((F, F)) * 0.1).astype(np.float32)}


def in_numbers(n, pattern="uniform", vocab=VOCAB, i64=False, seed=0):
    """Node numbers (n) as float32 or int64.  "uniform": over the vocabulary; "same": one number for every node; "ends":
    0 and vocab - 1 in turn; "oob": uniform with -1, vocab, 1000 (int64: and 2^31 + 3) spread over the rows from row 2 on;
    "fractional" (float32): uniform with 5.7, 94.5, -0.5 in between; "oob-last" / "oob-first": uniform with ``vocab`` on
    the last row / -1 on row 0."""
    rng = np.random.default_rng(9800 + 7 * seed + n + 100003 * vocab)
    z = rng.integers(0, vocab, size=n).astype(np.float64)
    if pattern == "same":
        z[:] = min(6, vocab - 1)
    elif pattern == "ends":
        z[0::2], z[1::2] = 0, vocab - 1
    elif pattern in ("oob", "fractional"):
        special = FRACTIONS if pattern == "fractional" else (OOB_NUMBERS_I64 if i64 else OOB_NUMBERS)
        rows = np.arange(2 % n, n, max(1, n // 7))
        for k, r in enumerate(rows):
            v = special[k % len(special)]
            z[r] = vocab if v == "vocab" else v
    elif pattern == "oob-last":
        z[n - 1] = vocab
    elif pattern == "oob-first":
        z[0] = -1
    elif pattern != "uniform":
        raise KeyError(pattern)
    return z.astype(np.int64) if i64 else z.astype(np.float32)


def in_case(n, emb_dim=64, pattern="uniform", vocab=VOCAB, bias=True, i64=False, seed=0):
    c = in_weights(emb_dim, vocab, seed)
    if not bias:
        c["b0"] = None
    c.update(N=n, pattern=pattern, i64=i64, numbers=in_numbers(n, pattern, vocab, i64, seed))
    return c


def in_rows(c):
    """(z, valid): the int32 truncation of every node number (Keras Embedding casts its input to int32; an int64 number
    keeps its low 32 bits) and whether it names a row of the embedding."""
    z = np.trunc(c["numbers"]).astype(np.int64).astype(np.int32)
    return z, (z >= 0) & (z < c["vocab"])


def in_restate(c, dtype):
    """``n = emb[z] W0 + b0 ; x = n Wx``; a number outside ``[0, vocab)`` reads a zero embedding row (what ``stage_load``
    does), so its ``n`` is ``b0``."""
    z, valid = in_rows(c)
    e = np.where(valid[:, None], c["emb"].astype(dtype)[np.clip(z, 0, c["vocab"] - 1)], np.dtype(dtype).type(0))
    n = e @ c["W0"].astype(dtype)
    if c["b0"] is not None:
        n = n + c["b0"].astype(dtype)
    return {"n": n.astype(dtype), "x": (n @ c["Wx"].astype(dtype)).astype(dtype)}


# ---------------------------------------------------------------------------------- C. stage 0
STAGE0_MAX_TILES = 1024      # mp_schnet_stage0_f32: tiles16 > 1024 -> two launches
STAGE0_MAX_GRAPHS = 1023     # mp_prep::PREP_LDS_GRAPHS
STAGE0_FLAGS = (PACKED | FAST, PACKED | FAST | BF)
EDGE_BLOCK = 256             # mp::grid_for: edges per workgroup of the edge role
EDGE_BLOCKS_BF_CAP = 64      # launch_stage0: the eight-wave build halves the edge workgroups and keeps at most 64


def stage0_fused(n, m, g):
    """True where mp_schnet_stage0_f32 runs both roles in one launch."""
    return not (n == 0 or m == 0 or tiles(n) > STAGE0_MAX_TILES or g > STAGE0_MAX_GRAPHS)


def stage0_edge_blocks_bf(m):
    """Edge workgroups of the eight-wave launch (before the cap, the cap applied)."""
    blocks = -(-m // EDGE_BLOCK)
    return (blocks + 1) // 2, min((blocks + 1) // 2, EDGE_BLOCKS_BF_CAP)


def stage0_batch(sizes, edges, seed=0):
    """A flat batch in the layout of ``synth.qm9_like_batch``: graphs of ``sizes`` nodes with ``edges`` random pairs each
    (a number, or one per graph), local ids, sorted by receiver; numbers 1..9 as float32, coordinates in N(0, 1.5^2)."""
    rng = np.random.default_rng(9900 + seed)
    sizes = np.asarray(sizes, np.int64)
    per = np.broadcast_to(np.asarray(edges, np.int64), sizes.shape)
    per = np.where(sizes > 0, per, 0)
    es = []
    for n, m in zip(sizes, per):
        recv = np.sort(rng.integers(0, max(n, 1), size=m))
        es.append(np.stack([recv, rng.integers(0, max(n, 1), size=m)], axis=-1).reshape(-1, 2))
    total = int(sizes.sum())
    splits = lambda lens: np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return {"node_number": rng.integers(1, 10, size=total).astype(np.float32),
            "node_coordinates": rng.normal(0.0, 1.5, size=(total, 3)).astype(np.float32),
            "edge_indices": np.concatenate(es, axis=0).reshape(-1, 2).astype(np.int64) if len(es) else
            np.zeros((0, 2), np.int64), "node_splits": splits(sizes), "edge_splits": splits(per)}


def _split_nodes(n, graphs):
    base = np.full(graphs, n // graphs, np.int64)
    base[:n % graphs] += 1
    return base


def stage0_cases():
    """name -> (batch builder, fused side expected).  The thresholds from the code's constants: 1024 tiles against 1025,
    1023 graphs against 1024 (single-node graphs, one self edge each), no edges, no nodes; and 4097 nodes with 300
    edges, where a node workgroup of the bf16-piece build takes a second tile beside the edge workgroups."""
    return {
        "second-tile": (lambda: stage0_batch(_split_nodes(TRIP_BF, 7), [60, 0, 100, 1, 39, 0, 100], seed=1), True),
        "second-tile-half-grid": (lambda: stage0_batch(_split_nodes(HALF_TWO, 5), 60, seed=2), True),
        "tiles-1024": (lambda: stage0_batch(_split_nodes(STAGE0_MAX_TILES * TILE, 4), 75, seed=3), True),
        "tiles-1025": (lambda: stage0_batch(_split_nodes(STAGE0_MAX_TILES * TILE + 1, 4), 75, seed=3), False),
        "graphs-1023": (lambda: stage0_batch(np.ones(STAGE0_MAX_GRAPHS, np.int64), 1, seed=4), True),
        "graphs-1024": (lambda: stage0_batch(np.ones(STAGE0_MAX_GRAPHS + 1, np.int64), 1, seed=4), False),
        "no-edges": (lambda: stage0_batch([9, 17, 3], 0, seed=5), False),
        "no-nodes": (lambda: stage0_batch([0], 0, seed=6), False),
    }


# ---------------------------------------------------------------------------------- D. layer-path build
RESIDUAL_COUNTS = EDGE_COUNTS + (TRIP_FP32,)
RESIDUAL_RUNS = [(n, True, False) for n in RESIDUAL_COUNTS] + [(TILE + 1, False, False), (TRIP_FP32, False, False),
                                                               (SATURATED_N, True, True)]


def residual_restate(c, dtype):
    """``n_out = n_in + ssp(agg W2 + b2) W3 + b3``: the ``n`` of ``node_restate`` (SchNetInteraction's node side)."""
    return node_restate(c, dtype)["n"]


# ---------------------------------------------------------------------------------- E. pack kernels
PACK_SHAPES = ((64, 128), (128, 128), (128, 64))


def pack_weights(k, u, seed=0):
    """(k, u) float32: N(0, 1) * 0.05 * 10^U(-4, 2) - six orders of magnitude, both signs - with one element in 17 set
    to exactly 0 (the ``wide_range`` recipe of test_node_kernels_on_the_bf16_pipe_keep_the_fp32_error_budget)."""
    rng = np.random.default_rng(9950 + seed + 7 * k + u)
    w = rng.standard_normal((k, u)) * (10.0 ** rng.uniform(-4, 2, size=(k, u))) * 0.05
    w = w.astype(np.float32)
    w.reshape(-1)[::17] = 0.0
    return w


def pack_index(k_rows, u):
    """(k, col) of every element i of the mp_schnet_node_pack_f32 image, from the comment above node_pack_kernel:
    ``i = (((w * NCB + cb) * (K/16) + q) * 64 + lane) * 4 + j`` holds
    ``W[4 * (4 q + j) + (lane >> 4)][w * (U/4) + 16 cb + (lane & 15)]`` with ``NCB = U / 64``."""
    ncb = u // 64
    i = np.arange(k_rows * u)
    j, lane, rest = i & 3, (i >> 2) & 63, i >> 8
    q, rest = rest % (k_rows // 16), rest // (k_rows // 16)
    cb, w = rest % ncb, rest // ncb
    return 4 * (4 * q + j) + (lane >> 4), w * (u // 4) + 16 * cb + (lane & 15)


def pack_restate(w):
    k, col = pack_index(*w.shape)
    return w[k, col]


def pack_bf16_index(k_rows, u):
    """(piece, k, col) of every 16-bit half h of the mp_schnet_node_pack_bf16_f32 image (h = 2 * dword + e, little
    endian), from the comment above node_pack_bf16_kernel: 16 B per (wave w, column block cb, k block kb, piece, lane),
    dword d of them holds elements ``2 d`` (low half) and ``2 d + 1`` of ``piece(W[32 kb + 8 (lane >> 4) + element]
    [w (U/4) + 16 cb + (lane & 15)])``."""
    ncb = u // 64
    h = np.arange(k_rows * u * 3)
    e, i = h & 1, h >> 1
    d, lane, rest = i & 3, (i >> 2) & 63, i >> 8
    pc, rest = rest % 3, rest // 3
    kb, rest = rest % (k_rows // 32), rest // (k_rows // 32)
    cb, w = rest % ncb, rest // ncb
    return pc, 32 * kb + 8 * (lane >> 4) + 2 * d + e, w * (u // 4) + 16 * cb + (lane & 15)


def _bf16(x):
    """float32 array -> (bf16 bits as uint16, the bf16 values as float32), torch's round-to-nearest-even on the CPU."""
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16)
    return t.view(torch.int16).numpy().view(np.uint16), t.to(torch.float32).numpy()


def bf16_split(w):
    """The split stated at mp_bf16_piece_bits: ``hi = bf16(x)``, ``mid = bf16(x - hi)``, ``lo = bf16(x - hi - mid)``, the
    differences in float32.  Returns (bits (3, K, U) uint16, values (3, K, U) float32)."""
    w = np.asarray(w, np.float32)
    b0, p0 = _bf16(w)
    r1 = w - p0
    b1, p1 = _bf16(r1)
    b2, p2 = _bf16(r1 - p1)
    return np.stack([b0, b1, b2]), np.stack([p0, p1, p2])


def pack_bf16_restate(w):
    """The image as uint16 halves."""
    bits, _ = bf16_split(w)
    pc, k, col = pack_bf16_index(*w.shape)
    return bits[pc, k, col]


def pack_bf16_decode(halves, k_rows, u):
    """uint16 halves of an image -> piece values (3, K, U) as float32."""
    pc, k, col = pack_bf16_index(k_rows, u)
    bits = np.zeros((3, k_rows, u), np.uint16)
    bits[pc, k, col] = np.asarray(halves, np.uint16)
    return (bits.astype(np.uint32) << 16).view(np.float32)
