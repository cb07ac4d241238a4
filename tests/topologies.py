"""Index lists off the molecular shapes, and the cases the shape-edge tests run on them.

The ``synth.*_batch`` generators only make small, fully connected molecules; the kernels branch on degree, tile
boundaries and table widths.  The first half of this module generates *index lists* with prescribed shapes (hub
receivers, exact tile sizes, hub edges of the triplet step, batches with empty graphs); the second half builds the
inputs, weights and torch restatements (float32 and float64) of every case tests/test_gpu_shape_edges.py runs, without
any engine import, so tests/test_topologies.py can check on the CPU that the generators deliver what they claim and
that each case's float32 restatement is itself inside the cap the GPU test applies.  Everything is seeded."""
import numpy as np
import torch

import egnn_reference as eref
import hdnnp_reference as href

TILE = 32   # edges per tile of csrc/mp_egnn.hip (TE)

# in-degrees in receiver order.  Cumulative ends 31, 32, 64, 97, 104, 168, 233, 333, 1333: the receiver of degree 1 ends
# exactly on a tile boundary, the one of degree 32 starts and ends on one, the one of degree 1000 covers 30 whole tiles
STANDARD_DEGREES = (31, 1, 32, 33, 7, 64, 65, 100, 1000)
SMALL_DEGREES = (31, 1, 32, 33, 7, 100)            # the same boundary placements, one receiver over four tiles
TILE_EXACT_SIZES = (0, 1, 31, 32, 33, 64)
# triplets per receiving edge: remainders 0, 1 and 7 modulo the 8-triplet step, one and several 64-lane rounds
STANDARD_TRIPLET_COUNTS = (0, 1, 7, 8, 9, 64, 65, 257, 1000)


# ------------------------------------------------------------------------------------------------------- generators
def _spread(n, count):
    """``count`` ascending row numbers inside ``[1, n - 1)``: rows 0 and n - 1 and the rows between stay untouched."""
    assert n >= 2 * count + 2, (n, count)
    return 1 + ((n - 2) // count) * np.arange(count)


def hub_edges(n, degrees, seed, self_loops=False, duplicates=False, order="sorted"):
    """Edge list ``(E, 2)`` int64 ``[receiver, sender]`` of one graph of ``n`` nodes: ``len(degrees)`` receivers
    (ascending, spread over the graph) with exactly these in-degrees, every other node isolated as a receiver; senders
    drawn at random among the other nodes (a degree above ``n - 1`` repeats senders).  ``self_loops``: every receiver of
    degree >= 2 also sends to itself once; ``duplicates``: every receiver of degree >= 3 lists one sender twice.  ``order``: "sorted" by receiver or
    "shuffled"."""
    rng = np.random.default_rng(seed)
    rows = []
    for r, deg in zip(_spread(n, len(degrees)), degrees):
        others = np.delete(np.arange(n), r)
        s = rng.choice(others, size=deg, replace=deg > len(others))
        if self_loops and deg >= 2:
            s[0] = r
        if duplicates and deg >= 3:
            s[2] = s[1]
        rows.append(np.stack([np.full(deg, r), s], axis=-1))
    e = np.concatenate(rows, axis=0).astype(np.int64).reshape(-1, 2) if rows else np.zeros((0, 2), np.int64)
    if order == "shuffled":
        e = e[rng.permutation(len(e))]
    else:
        assert order == "sorted", order
    return e


def degree_edges(n, degrees, seed, first=0):
    """Edge list ``(E, 2)`` int64 ``[receiver, sender]``, sorted by receiver, of one graph of ``n`` nodes: the CONSECUTIVE
    nodes ``first, first + 1, ...`` have exactly these in-degrees (0 allowed), every other node receives nothing; senders
    drawn at random among the other nodes (a degree above ``n - 1`` repeats senders).  ``hub_edges`` spreads its
    receivers; kernels that walk receivers in pairs or tiles need the degrees side by side."""
    assert first >= 0 and first + len(degrees) <= n, (n, first, len(degrees))
    rng = np.random.default_rng(seed)
    rows = [np.zeros((0, 2), np.int64)]
    for k, deg in enumerate(degrees):
        others = np.delete(np.arange(n), first + k)
        s = rng.choice(others, size=deg, replace=deg > len(others))
        rows.append(np.stack([np.full(deg, first + k), s], axis=-1).astype(np.int64).reshape(-1, 2))
    return np.concatenate(rows, axis=0)


def two_neighbour_edges(n):
    """Edge list sorted by receiver in which node ``i`` of ``n >= 3`` receives from ``i + 1`` and ``i + 2`` (modulo ``n``):
    degree 2 on both columns, no self loops."""
    assert n >= 3, n
    i = np.repeat(np.arange(n), 2)
    return np.stack([i, (i + np.tile([1, 2], n)) % n], axis=-1).astype(np.int64)


def tile_exact(total, n=5, seed=0):
    """``(n, edges)``: a graph of ``n`` nodes with exactly ``total`` edges, sorted by receiver (``total = 0``: nodes
    only, the finishing pass alone runs)."""
    rng = np.random.default_rng(seed + total)
    recv = np.sort(rng.integers(0, n, size=total))
    send = (recv + rng.integers(1, n, size=total)) % n
    return n, np.stack([recv, send], axis=-1).astype(np.int64).reshape(-1, 2)


def swap_columns(edges):
    """The same pairs with receiver and sender exchanged: a list sorted by receiver becomes one sorted by sender, and the
    in-degrees of the first column become those of the second."""
    return np.ascontiguousarray(np.asarray(edges)[:, ::-1])


def ring_edges(n, step):
    """Edge list ``(E, 2)`` int64, sorted by receiver, of a ring over every ``step``-th node of ``n``: node ``step * k``
    receives from its successor on the ring (the last one from node 0); every other node is isolated on both columns."""
    assert step >= 2 and n > 2 * step, (n, step)
    ring = np.arange(0, n, step)
    return np.stack([ring, np.roll(ring, -1)], axis=-1).astype(np.int64).reshape(-1, 2)


def hub_triplets(num_edges, counts, seed, order="sorted"):
    """Angle pairs ``(T, 2)`` int64 ``[n, m]`` over ``num_edges`` edges: ``len(counts)`` receiving edges ``n`` (ascending,
    spread) with exactly these numbers of triplets, partners ``m != n`` drawn at random; other edges receive none."""
    rng = np.random.default_rng(seed)
    rows = []
    for e, c in zip(_spread(num_edges, len(counts)), counts):
        m = rng.choice(np.delete(np.arange(num_edges), e), size=c, replace=c >= num_edges)
        rows.append(np.stack([np.full(c, e), m], axis=-1))
    a = np.concatenate(rows, axis=0).astype(np.int64).reshape(-1, 2)
    if order == "shuffled":
        a = a[rng.permutation(len(a))]
    else:
        assert order == "sorted", order
    return a


def with_empty_graphs(graphs):
    """``graphs``: list of ``(rows, index)``; the same list with an empty graph first, in the middle and last."""
    width = graphs[0][1].shape[1]
    empty = (0, np.zeros((0, width), np.int64))
    mid = (len(graphs) + 1) // 2
    return [empty] + list(graphs[:mid]) + [empty] + list(graphs[mid:]) + [empty]


def batch(graphs):
    """Ragged batch of ``(rows, index)`` graphs: ``row_splits``, ``index_splits``, ``indices`` (local to each graph, what
    the layers take) and ``flat`` (shifted into the batch, what the restatements take)."""
    rows = np.array([g[0] for g in graphs], np.int64)
    lens = np.array([len(g[1]) for g in graphs], np.int64)
    rs = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    local = np.concatenate([g[1] for g in graphs], axis=0).astype(np.int64)
    flat = local + np.repeat(rs[:-1], lens)[:, None]
    return {"row_splits": rs, "index_splits": np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
            "indices": local, "flat": flat}


def in_degrees(flat, rows, column=0):
    return np.bincount(flat[:, column], minlength=rows)


def tile_placement(flat, rows, tile=TILE):
    """Where the receivers' edge ranges (in receiver order, as the CSR holds them) fall against ``tile``-edge tiles:
    how many start exactly on a boundary, how many end exactly on one, the largest number of WHOLE tiles inside one
    receiver's range and the largest number of tiles one range touches."""
    deg = in_degrees(flat, rows)
    ptr = np.concatenate([[0], np.cumsum(deg)])
    lo, hi = ptr[:-1][deg > 0], ptr[1:][deg > 0]
    whole = np.maximum(hi // tile - -(-lo // tile), 0)
    return {"starts_on_boundary": int(np.sum(lo % tile == 0)), "ends_on_boundary": int(np.sum(hi % tile == 0)),
            "max_whole_tiles": int(whole.max()) if len(whole) else 0,
            "max_tiles_touched": int(((hi - 1) // tile - lo // tile + 1).max()) if len(lo) else 0}


def points(rng, n, sigma, min_distance=0.9):
    """``n`` positions N(0, sigma^2), each redrawn until ``min_distance`` from the earlier ones."""
    xyz = np.zeros((n, 3))
    for a in range(n):
        while True:
            p = rng.normal(0.0, sigma, size=3)
            if a == 0 or np.min(np.linalg.norm(xyz[:a] - p, axis=-1)) >= min_distance:
                break
        xyz[a] = p
    return xyz


def all_pairs(n):
    return np.array([[a, c] for a in range(n) for c in range(n) if a != c], np.int64).reshape(-1, 2)


def all_triplets(n):
    """Every ``(i, j, k)`` of distinct atoms, sorted by ``i``."""
    i, j, k = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    keep = (i != j) & (i != k) & (j != k)
    return np.stack([i[keep], j[keep], k[keep]], axis=-1).astype(np.int64).reshape(-1, 3)


def _glorot(rng, fan_in, fan_out):
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-lim, lim, size=(fan_in, fan_out)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------- EGNN cases
F = 128   # node and message width of the fused edge step


def egnn_graphs(kind, order="sorted", selfdup=False, seed=0):
    if kind == "hub":      # 200 + 60 nodes around the empty graphs
        big = (200, hub_edges(200, STANDARD_DEGREES, seed, selfdup, selfdup, order))
        small = (60, hub_edges(60, (2, 96, 5), seed + 1, selfdup, selfdup, order))
        return with_empty_graphs([big, small])
    if kind == "small_hub":
        return with_empty_graphs([(40, hub_edges(40, SMALL_DEGREES, seed, order=order)), (3, all_pairs(3))])
    if kind.startswith("exact"):
        return [tile_exact(int(kind[5:]), seed=seed)]
    raise KeyError(kind)


def one_frequency_scales():
    """The single scale of the one-frequency encoding (K = 1; PositionEncodingBasisLayer itself starts at dim_half 2)."""
    return np.array([2.0 * np.pi], np.float32)


def egnn_scales(dim_half):
    if dim_half == 0:
        return None
    return one_frequency_scales() if dim_half == 1 else eref.encoding_scales(dim_half)


def egnn_case(kind="hub", order="sorted", attention=True, dim_half=10, interleave=False, selfdup=False,
              acts=("swish", "swish"), gate="sigmoid", bias=(True, True, True), seed=0, d_max=10.0):
    """Inputs and weights of one fused-edge-step case: ``h`` (N, 128), ``x = d^2`` (E, 1) with ``d`` in 0.9..``d_max``,
    the upstream gradient ``g`` (N, 128), Glorot kernels and biases in +-0.1 (``bias`` switches those of the first
    layer, the second layer and the gate off)."""
    b = batch(egnn_graphs(kind, order, selfdup, seed))
    rng = np.random.default_rng(1000 + seed)
    n, e = int(b["row_splits"][-1]), len(b["flat"])
    cols = 2 * dim_half if dim_half else 1
    small = lambda size: rng.uniform(-0.1, 0.1, size=size).astype(np.float32)
    w = {"w1": _glorot(rng, 2 * F + cols, F), "b1": small(F) if bias[0] else None,
         "w2": _glorot(rng, F, F), "b2": small(F) if bias[1] else None,
         "wa": _glorot(rng, F, 1) if attention else None, "ba": small(1) if attention and bias[2] else None}
    b.update(h=rng.normal(size=(n, F)).astype(np.float32),
             x=(rng.uniform(0.9, d_max, size=(e, 1)) ** 2).astype(np.float32),
             g=rng.normal(size=(n, F)).astype(np.float32), weights=w, attention=attention, dim_half=dim_half,
             interleave=interleave, acts=tuple(acts), gate=gate, rows=n)
    return b


def egnn_restate(case, dtype):
    """(m_i, h_bar, x_bar) of the edge step (egnn_reference.edge_step on the case's encoding), numpy."""
    t = lambda a: None if a is None else torch.tensor(a, dtype=dtype)
    w = case["weights"]
    h = t(case["h"]).requires_grad_(True)
    x = t(case["x"]).requires_grad_(True)
    enc = x
    if case["dim_half"]:
        arg = x * t(egnn_scales(case["dim_half"]))[None, :]
        pair = [torch.sin(arg), torch.cos(arg)]
        enc = torch.stack(pair, dim=-1).reshape(arg.shape[0], -1) if case["interleave"] else torch.cat(pair, dim=-1)
    edge_mlp = [(t(w["w1"]), t(w["b1"]), case["acts"][0]), (t(w["w2"]), t(w["b2"]), case["acts"][1])]
    att = [(t(w["wa"]), t(w["ba"]), case["gate"])] if case["attention"] else None
    _, m_i = eref.edge_step(h, enc, torch.from_numpy(case["flat"]), edge_mlp, att, dtype)
    if len(case["flat"]) == 0:
        return m_i.detach().numpy(), np.zeros_like(case["h"], dtype=np.float64), np.zeros_like(case["x"], np.float64)
    gh, gx = torch.autograd.grad(m_i, [h, x], t(case["g"]))
    return m_i.detach().numpy(), gh.numpy(), gx.numpy()


# the model-level case: a 70-atom molecule whose atoms all have 66 to 69 neighbours (three tiles per receiver), a lone
# atom, an empty graph and an aspirin-sized molecule.  Cutoff 8 A on a compact molecule (sigma 1.2) for the reason
# tests/test_gpu_egnn.py gives on 6 A against 10 A: the float32 restatement's forces stay 5e-06 / 1e-05 of the molecule's
# scale from float64, against 1.5e-05 at sigma 1.7 and 10 A
EGNN_MODEL_BATCH = dict(sizes=[70, 1, 0, 21], seed=22, min_distance=0.9, max_distance=8.0, sigma=1.2)

HIDDEN_ACTIVATIONS = ("relu", "tanh", "softplus", "shifted_softplus", "leaky_relu", "selu")
GATE_ACTIVATIONS = ("sigmoid", "tanh", "linear")


def egnn_cases():
    """name -> keyword arguments of ``egnn_case`` for every edge-step case of the GPU tests."""
    out = {}
    for order in ("sorted", "shuffled"):
        for att in (True, False):
            for enc in (True, False):
                # without the encoding x_bar is a cancelling 128-term dot product with W_c whose float32 noise is
                # independent in every pipeline (with it, all share the rounding of the sine arguments): seed 13 keeps
                # the engine, the layer sequence and the restatement clear of each other's noise on all four variants
                out["hub-%s-att%d-enc%d" % (order, att, enc)] = dict(kind="hub", order=order, attention=att,
                                                                     dim_half=10 if enc else 0, seed=3 if enc else 13)
    out["hub-selfdup"] = dict(kind="hub", selfdup=True, seed=9)
    for e in TILE_EXACT_SIZES:
        out["exact%d" % e] = dict(kind="exact%d" % e, seed=5)
    for dim_half in (1, 10, 32, 0):
        for inter in ((False, True) if dim_half else (False,)):
            out["width%d-il%d" % (dim_half, inter)] = dict(kind="small_hub", dim_half=dim_half, interleave=inter,
                                                           seed=6 if dim_half else 21)
    out["width33"] = dict(kind="small_hub", dim_half=33, seed=6)       # beyond the fused step: the layer sequence
    for k, act in enumerate(HIDDEN_ACTIVATIONS):
        out["act-%s" % act] = dict(kind="small_hub", acts=(act, HIDDEN_ACTIVATIONS[(k + 1) % len(HIDDEN_ACTIVATIONS)]),
                                   gate=GATE_ACTIVATIONS[k % 3], seed=9)
    for k in range(3):
        out["nobias%d" % k] = dict(kind="small_hub", bias=tuple(i != k for i in range(3)), seed=9)
    return out


# ------------------------------------------------------------------------------------------------------- DimeNet++ cases
TRIPLET_WIDTHS = (1, 7, 42, 64)


def triplet_case(nsbf, order="sorted", seed=0):
    """The triplet step on hub edges: 300 + 24 edges around empty graphs, ``xdown`` (E, 64), a random ``sbf`` (T, nsbf),
    ``W_sbf1`` (nsbf, 8) and ``W_sbf2`` (8, 64) in +-0.3, upstream gradient ``g`` (E, 64)."""
    graphs = with_empty_graphs([(300, hub_triplets(300, STANDARD_TRIPLET_COUNTS, seed, order)),
                                (24, hub_triplets(24, (3, 0, 16, 66), seed + 1, order))])
    b = batch(graphs)
    rng = np.random.default_rng(2000 + seed)
    e, t = int(b["row_splits"][-1]), len(b["flat"])
    b.update(xdown=rng.normal(size=(e, 64)).astype(np.float32),
             sbf=rng.uniform(-1, 1, size=(t, nsbf)).astype(np.float32),
             w1=rng.uniform(-0.3, 0.3, size=(nsbf, 8)).astype(np.float32),
             w2=rng.uniform(-0.3, 0.3, size=(8, 64)).astype(np.float32),
             g=rng.normal(size=(e, 64)).astype(np.float32), rows=e, nsbf=nsbf)
    if nsbf == 1:
        # a one-column sbf_bar row is ONE sum of 64 x 8 products; with signed factors the worst of 1500 such scalars
        # cancels to where any float32 evaluation is 2e-05..6e-05 of it from float64 (13 seeds), at or over half the cap.
        # Positive xdown, g and W_sbf2 leave the signs to W_sbf1 alone: every row cancels alike, by sum(w1) / sum|w1|
        b.update(xdown=rng.uniform(0.5, 1.5, size=(e, 64)).astype(np.float32),
                 g=rng.uniform(0.5, 1.5, size=(e, 64)).astype(np.float32),
                 w2=rng.uniform(0.05, 0.3, size=(8, 64)).astype(np.float32))
    return b


def triplet_restate(case, dtype):
    """(out, xdown_bar, sbf_bar): ``sum_{t: A[t,0] = n} xdown[A[t,1]] * ((sbf_t W1) W2)`` and its reverse."""
    t = lambda a: torch.tensor(a, dtype=dtype)
    x, s = t(case["xdown"]).requires_grad_(True), t(case["sbf"]).requires_grad_(True)
    a = torch.from_numpy(case["flat"])
    trip = x[a[:, 1]] * ((s @ t(case["w1"])) @ t(case["w2"]))
    out = torch.zeros((x.shape[0], 64), dtype=dtype).index_add(0, a[:, 0], trip)
    gx, gs = torch.autograd.grad(out, [x, s], t(case["g"]))
    return out.detach().numpy(), gx.numpy(), gs.numpy()


def many_triplets_batch(shuffled=False, seed=33):
    """Real geometry whose edges carry more than 64 triplets: a 72-atom all-connected molecule (70 per edge), a 3-atom
    one and a lone atom; the angle lists sorted or shuffled inside each molecule."""
    from gcnn_keras_amd import synth
    b = synth.dimenet_batch(sizes=[72, 3, 1], seed=seed, min_distance=0.9, max_distance=30.0, sigma=1.2)
    if shuffled:
        rng = np.random.default_rng(7)
        a, s = b["angle_indices"].copy(), b["angle_splits"]
        for g in range(len(s) - 1):
            a[s[g]:s[g + 1]] = a[s[g]:s[g + 1]][rng.permutation(s[g + 1] - s[g])]
        b["angle_indices"] = a
    return b


# ------------------------------------------------------------------------------------------------------- ACSF cases
ELEMENTS = (1, 6, 8)


def g2_table(nrel, nfun, seed, ncenter=0, rc=(6.0, 20.0)):
    """``(nrel, nfun, 3)`` (or with ``ncenter`` leading) rows ``(eta, rs, rc)``, every function its own cutoff."""
    rng = np.random.default_rng(seed)
    shape = ((ncenter,) if ncenter else ()) + (nrel, nfun)
    t = np.stack([rng.uniform(0.01, 0.5, size=shape), rng.uniform(0.0, 4.0, size=shape),
                  rng.uniform(rc[0], rc[1], size=shape)], axis=-1)
    return t.astype(np.float32).astype(np.float64)       # float32-exact entries: both precisions read the same table


def g4_table(nrel, nfun, seed, ncenter=0, rc=(6.0, 12.0)):
    """Rows ``(eta, zeta, lambda, rc)``: zeta in {1, 2, 4, 8, 16}, lambda = +-1, every function its own cutoff."""
    rng = np.random.default_rng(seed)
    shape = ((ncenter,) if ncenter else ()) + (nrel, nfun)
    t = np.stack([rng.uniform(0.001, 0.05, size=shape), rng.choice([1.0, 2.0, 4.0, 8.0, 16.0], size=shape),
                  rng.choice([-1.0, 1.0], size=shape), rng.uniform(rc[0], rc[1], size=shape)], axis=-1)
    return t.astype(np.float32).astype(np.float64)


def acsf_batch(sizes, seed, sigma=1.8, triplets=True, elements=ELEMENTS, pair_lists=None):
    """Molecules of ``sizes`` atoms (0 allowed) with all pairs ``(i, j)`` and, with ``triplets``, all ``(i, j, k)``;
    ``pair_lists`` replaces the pair lists.  Global copies ``ij`` / ``ijk`` for the restatements."""
    rng = np.random.default_rng(seed)
    xs = [points(rng, n, sigma) for n in sizes]
    pairs = pair_lists if pair_lists is not None else [all_pairs(n) for n in sizes]
    trips = [all_triplets(n) if triplets else np.zeros((0, 3), np.int64) for n in sizes]
    ns = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    z = rng.choice(np.array(elements), size=int(ns[-1])).astype(np.int64)
    b = {"node_number": z, "node_coordinates": np.concatenate(xs, axis=0).astype(np.float32).reshape(-1, 3),
         "node_splits": ns, "edge_indices": np.concatenate(pairs, axis=0).reshape(-1, 2),
         "edge_splits": np.concatenate([[0], np.cumsum([len(p) for p in pairs])]).astype(np.int64),
         "angle_indices": np.concatenate(trips, axis=0).reshape(-1, 3),
         "angle_splits": np.concatenate([[0], np.cumsum([len(p) for p in trips])]).astype(np.int64)}
    b["ij"] = b["edge_indices"] + np.repeat(ns[:-1], np.diff(b["edge_splits"]))[:, None]
    b["ijk"] = b["angle_indices"] + np.repeat(ns[:-1], np.diff(b["angle_splits"]))[:, None]
    return b


def pair_maps(elements):
    """(rmap, pmap, number of pair relations) as ACSFG4 builds them for unordered pairs of sorted ``elements``."""
    el = sorted(elements)
    rmap = {z: s for s, z in enumerate(el)}
    pmap, nxt = {}, 0
    for a in range(len(el)):                      # entry a*n + b is (element b, element a), sorted, first appearance
        for c in range(len(el)):
            key = tuple(sorted((el[c], el[a])))
            if key not in pmap:
                pmap[key] = nxt
                nxt += 1
    full = {}
    for (p, q), r in pmap.items():
        full[(p, q)] = r
        full[(q, p)] = r
    return rmap, full, nxt


def acsf_restate(kind, b, table, dtype, elements=ELEMENTS, multiplicity=None, jvp=None, g=None):
    """Forward (N, R*m); with ``g`` also the reverse ``dx``; with ``jvp`` = h also ``g_bar`` (the adjoint's backward)."""
    rmap, pmap, npair = pair_maps(elements)
    ncenter = table.shape[0] if table.ndim == 4 else 0
    x = torch.tensor(b["node_coordinates"], dtype=dtype).requires_grad_(g is not None)
    if kind == "g2":
        out = href.g2(b["node_number"], x, b["ij"], table, rmap, len(rmap), ncenter)
    else:
        out = href.g4(b["node_number"], x, b["ijk"], table, rmap, pmap, npair, multiplicity, ncenter)
    if g is None:
        return (out.detach().numpy(),)
    gg = torch.tensor(g, dtype=dtype).requires_grad_(jvp is not None)
    dx, = torch.autograd.grad(out, x, grad_outputs=gg, create_graph=jvp is not None)
    if jvp is None:
        return out.detach().numpy(), dx.detach().numpy()
    gb, = torch.autograd.grad(dx, gg, grad_outputs=torch.tensor(jvp, dtype=dtype))
    return out.detach().numpy(), dx.detach().numpy(), gb.detach().numpy()


def exact_pair_receivers():
    """One 67-atom graph in which atom 0 has exactly 64 pairs and atom 1 exactly 65 (one and two 64-pair rounds)."""
    return [np.array([[0, s] for s in range(1, 65)] + [[1, s] for s in [0] + list(range(2, 66))], np.int64)]


def acsf_cases():
    """name -> (kind, batch, table, multiplicity, with_jvp) of every ACSF case of the GPU tests."""
    out = {}
    sizes = [0, 9, 1, 0, 12, 2, 0]
    for kind, nfun in (("g2", 70), ("g4", 100)):
        for target in (False, True):
            nrel = 3 if kind == "g2" else 6
            make = g2_table if kind == "g2" else g4_table
            out["wide-%s-%s" % (kind, "target" if target else "plain")] = (
                kind, acsf_batch(sizes, 41), make(nrel, nfun, 42, ncenter=3 if target else 0),
                2.0 if kind == "g4" else None, True)
    out["many-g2-150"] = ("g2", acsf_batch([150], 43, sigma=3.0, triplets=False), g2_table(3, 70, 44), None, False)
    out["many-g2-64-65"] = ("g2", acsf_batch([67], 45, sigma=2.5, triplets=False, pair_lists=exact_pair_receivers()),
                            g2_table(3, 70, 46), None, False)
    out["many-g4-40"] = ("g4", acsf_batch([40], 47, sigma=2.2), g4_table(6, 100, 48), 2.0, False)
    four = (1, 6, 7, 8)
    small = acsf_batch([0, 14, 1, 9], 49, triplets=False, elements=four)
    out["bound-g2-4x512"] = ("g2", small, g2_table(4, 512, 50), None, False)                 # R*m = 2048
    out["global-g2-4x171"] = ("g2", small, g2_table(4, 171, 51), None, False)               # table 2052 floats, R*m 684
    return out


def acsf_elements(name):
    return (1, 6, 7, 8) if name.startswith(("bound", "global")) else ELEMENTS


def acsf_upstream(name, b, width):
    """(g (N, width), h (N, 3)) float32 for the reverse and the JVP of a case."""
    rng = np.random.default_rng(sum(map(ord, name)))
    n = len(b["node_number"])
    return rng.normal(size=(n, width)).astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------- large graph
def large_graph_batch(n=5000, neighbours=12, seed=61):
    """One graph of ``n`` points on a jittered 1.7 A lattice, each receiving from its ``neighbours`` nearest points within
    5 A (receiver-sorted edge list), elements of aspirin cycled."""
    from gcnn_keras_amd import synth
    rng = np.random.default_rng(seed)
    side = int(np.ceil(n ** (1.0 / 3.0)))
    grid = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)[:n]
    xyz = (1.7 * grid + rng.uniform(-0.3, 0.3, size=(n, 3))).astype(np.float32)
    # nearest neighbours by blocks of rows (the full distance matrix of synth.radius_graph would be 200 MB)
    edges = []
    for lo in range(0, n, 500):
        d = np.linalg.norm(xyz[lo:lo + 500, None, :].astype(np.float64) - xyz[None, :, :], axis=-1)
        d[np.arange(len(d)), lo + np.arange(len(d))] = np.inf
        near = np.sort(np.argsort(d, axis=-1)[:, :neighbours], axis=-1)
        keep = np.take_along_axis(d, near, axis=-1) < 5.0
        recv = np.repeat(lo + np.arange(len(d)), neighbours).reshape(len(d), neighbours)
        edges.append(np.stack([recv[keep], near[keep]], axis=-1))
    e = np.concatenate(edges, axis=0).astype(np.int64)
    return {"node_number": np.resize(synth.ASPIRIN_Z, n).astype(np.float32), "node_coordinates": xyz,
            "node_splits": np.array([0, n], np.int64), "edge_indices": e, "edge_splits": np.array([0, len(e)], np.int64)}
