"""Differentiable torch-CPU restatement of MEGNet (kgcnn/literature/Megnet.py:118-193 and :292-373,
kgcnn/layers/conv/megnet_conv.py:96-120, kgcnn/layers/pool/set2set.py:172-263, kgcnn/layers/geom.py ShiftPeriodicLattice),
in float64 or float32: the budget and the float32 twin of the GPU tests.  TEST INFRASTRUCTURE: no engine imports.

Weights are consumed in ``model.weights`` order of ``gcnn_keras_amd.literature.Megnet``: the node embedding (with an
embedding input), the state embedding (with a ``shape: []`` state input), the first feed-forward triple (node, edge,
state MLP; kernel, bias per layer), then per block [with ``has_ff`` from the second block on: a feed-forward triple,]
the block's node, edge and state chains (three Dense each), with Set2Set the two Dense (kernel, bias) and the two
Set2Set (kernel, recurrent_kernel, bias), last the output MLP.  ``cfg`` is the merged keyword dictionary of the builder.

The mean of an empty segment (a receiver without edges, a graph without edges or nodes) is defined as 0.
"""
import numpy as np
import torch

from cgcnn_reference import flat_edges, gauss_basis, seg_sum

LN2 = float(np.log(2.0))
ACTIVATIONS = {
    None: lambda x: x, "linear": lambda x: x, "swish": lambda x: x * torch.sigmoid(x), "sigmoid": torch.sigmoid,
    "tanh": torch.tanh, "relu": torch.relu, "softplus": torch.nn.functional.softplus,
    # kgcnn/ops/activ.py:19-29: relu(x) + log(0.5 exp(-|x|) + 0.5) = softplus(x) - log 2, stable form
    "kgcnn>softplus2": lambda x: torch.relu(x) + torch.log(0.5 * torch.exp(-torch.abs(x)) + 0.5),
    "kgcnn>shifted_softplus": lambda x: torch.nn.functional.softplus(x) - LN2,
}


def _t(a, dtype):
    return a.to(dtype) if torch.is_tensor(a) else torch.tensor(np.asarray(a), dtype=dtype)


def graph_ids(splits):
    s = np.asarray(splits, np.int64)
    return torch.from_numpy(np.repeat(np.arange(len(s) - 1), s[1:] - s[:-1]))


def seg_pool(x, idx, rows, method):
    """Sum or mean of the rows of ``x`` per segment id; an empty segment gives 0 either way."""
    out = seg_sum(x, idx, rows)
    if method in ("mean", "segment_mean", "reduce_mean"):
        count = torch.bincount(idx, minlength=rows).to(x.dtype)
        return out / torch.clamp(count, min=1.0)[:, None]
    if method not in ("sum", "segment_sum", "reduce_sum"):
        raise ValueError(method)
    return out


def dense(x, it, activation, use_bias=True):
    y = x @ next(it)
    if use_bias:
        y = y + next(it)
    return ACTIVATIONS[activation](y)


def _listed(value, n):
    return list(value) if isinstance(value, (list, tuple)) else [value] * n


def mlp(x, it, args):
    units = _listed(args["units"], 1)
    acts, bias = _listed(args.get("activation"), len(units)), _listed(args.get("use_bias", True), len(units))
    for a, b in zip(acts, bias):
        x = dense(x, it, a, b)
    return x


def take_block_weights(it, use_bias=True):
    """The next MEGnetBlock's weights from an iterator in ``model.weights`` order: the node, edge and state chain, each
    a list of three ``(kernel, bias or None)``."""
    return {key: [(next(it), next(it) if use_bias else None) for _ in range(3)] for key in ("phi_n", "phi_e", "phi_u")}


def _chain(x, layers, activation):
    for k, (kernel, bias) in enumerate(layers):
        x = x @ kernel
        if bias is not None:
            x = x + bias
        x = ACTIVATIONS[activation if k < 2 else "linear"](x)
    return x


def megnet_block(v, e, ei, u, node_graph, edge_graph, w, activation="kgcnn>softplus2", pooling_method="mean"):
    """One MEGnetBlock (megnet_conv.py:96-120) on flat tensors: ``v`` (N, Fn), ``e`` (E, Fe), ``ei`` (E, 2) batch-shifted,
    ``u`` (G, Fu), the graph of every node and edge.  Returns ``(v', e', u')``."""
    n, g = v.shape[0], u.shape[0]
    ep = _chain(torch.cat([v[ei[:, 0]], v[ei[:, 1]], e, u[edge_graph]], dim=-1), w["phi_e"], activation)
    vb = seg_pool(ep, ei[:, 0], n, pooling_method)
    vp = _chain(torch.cat([vb, v, u[node_graph]], dim=-1), w["phi_n"], activation)
    es, vs = seg_pool(ep, edge_graph, g, pooling_method), seg_pool(vp, node_graph, g, pooling_method)
    up = _chain(torch.cat([es, vs, u], dim=-1), w["phi_u"], activation)
    return vp, ep, up


def set2set(m, graph, g, it, args):
    """PoolingSet2Set (set2set.py:172-263): a stateless one-step LSTM per round, so the recurrent kernel multiplies
    zeros; attention by a per-graph softmax of ``pool(m * q)``.  Returns ``(G, 2 * channels)``."""
    kernel, _, bias = next(it), next(it), next(it)
    f = m.shape[1]
    pool = (lambda x: x.mean(dim=1)) if args.get("pooling_method", "mean") == "mean" else (lambda x: x.sum(dim=1))

    def attend(q):
        et = pool(m * q[graph])
        mx = torch.full((g,), -float("inf"), dtype=m.dtype).scatter_reduce(0, graph, et.detach(), "amax")
        at = torch.exp(et - mx[graph])
        norm = seg_sum(at, graph, g)
        inv = torch.where(norm == 0, torch.zeros_like(norm), 1.0 / torch.where(norm == 0, torch.ones_like(norm), norm))
        return seg_sum(m * (inv[graph] * at)[:, None], graph, g)

    if args.get("init_qstar", "0") == "mean":
        q = seg_pool(m, graph, g, "mean")
        qstar = torch.cat([q, attend(q)], dim=1)
    else:
        qstar = torch.zeros((g, 2 * f), dtype=m.dtype)
    for _ in range(int(args.get("T", 3))):
        z = qstar @ kernel + bias
        zi, _, zc, zo = torch.split(z, f, dim=1)
        c = torch.sigmoid(zi) * torch.tanh(zc)
        q = torch.sigmoid(zo) * torch.tanh(c)
        qstar = torch.cat([q, attend(q)], dim=1)
    return qstar


def periodic_distances(b, dtype):
    """(E, 1): ``|x_i - (x_j + image @ lattice)|`` with the lattice vectors in rows (ShiftPeriodicLattice, then
    NodeDistanceEuclidean = sqrt(relu(sum of squares)))."""
    ei = torch.from_numpy(flat_edges(b))
    xyz, lattice = _t(b["node_coordinates"], dtype), _t(b["graph_lattice"], dtype)
    image = torch.from_numpy(np.asarray(b["edge_image"], np.int64)).to(dtype)
    rows = lattice[graph_ids(b["edge_splits"])]                      # (E, 3, 3)
    prod = rows * image.unsqueeze(-1)
    shift = (prod[:, 0] + prod[:, 1]) + prod[:, 2]
    diff = xyz[ei[:, 0]] - (xyz[ei[:, 1]] + shift)
    return torch.sqrt(torch.relu(diff.square().sum(-1, keepdim=True)))


def megnet_forward(weights, b, cfg, dtype=torch.float64, crystal=True):
    """(G, L) output of the model on batch ``b``: ``node_number`` (or ``node_attributes``), ``node_coordinates``,
    ``edge_indices``, ``state`` ((G,) numbers or (G, F) floats), ``edge_image``, ``graph_lattice`` and the splits;
    ``edge_distance`` with ``make_distance=False``.  Differentiable in ``weights`` when they are tensors."""
    it = iter([_t(w, dtype) for w in weights])
    ei = torch.from_numpy(flat_edges(b))
    node_graph, edge_graph = graph_ids(b["node_splits"]), graph_ids(b["edge_splits"])
    g = len(b["node_splits"]) - 1
    if len(cfg["inputs"][0]["shape"]) < 2:
        v = next(it)[torch.from_numpy(np.asarray(b["node_number"]).astype(np.int64))]
    else:
        v = _t(b["node_attributes"], dtype)
    if len(cfg["inputs"][3]["shape"]) < 1:
        u = next(it)[torch.from_numpy(np.asarray(b["state"]).astype(np.int64))]
    else:
        u = _t(b["state"], dtype).reshape(g, -1)
    if cfg["make_distance"]:
        if crystal:
            ed = periodic_distances(b, dtype)
        else:
            xyz = _t(b["node_coordinates"], dtype)
            ed = torch.sqrt(torch.relu((xyz[ei[:, 0]] - xyz[ei[:, 1]]).square().sum(-1, keepdim=True)))
    else:
        ed = _t(b["edge_distance"], dtype)
    if cfg["expand_distance"]:
        ed = gauss_basis(ed, cfg["gauss_args"], dtype)
    blk = cfg["meg_block_args"]
    act, pooling, use_bias = blk.get("activation", "kgcnn>softplus2"), blk.get("pooling_method", "mean"), \
        blk.get("use_bias", True)
    vp, ep, up = mlp(v, it, cfg["node_ff_args"]), mlp(ed, it, cfg["edge_ff_args"]), mlp(u, it, cfg["state_ff_args"])
    vp2, ep2, up2 = vp, ep, up
    for i in range(cfg["nblocks"]):
        if cfg["has_ff"] and i > 0:
            vp2, ep2, up2 = mlp(vp, it, cfg["node_ff_args"]), mlp(ep, it, cfg["edge_ff_args"]), \
                mlp(up, it, cfg["state_ff_args"])
        w = take_block_weights(it, use_bias)
        vp2, ep2, up2 = megnet_block(vp2, ep2, ei, up2, node_graph, edge_graph, w, act, pooling)
        vp, ep, up = vp2 + vp, ep2 + ep, up2 + up
    if cfg["use_set2set"]:
        s2s = cfg["set2set_args"]
        vd, ed2 = dense(vp, it, "linear"), dense(ep, it, "linear")
        vp, ep = set2set(vd, node_graph, g, it, s2s), set2set(ed2, edge_graph, g, it, s2s)
    else:
        vp, ep = seg_pool(vp, node_graph, g, "mean"), seg_pool(ep, edge_graph, g, "mean")
    out = mlp(torch.cat([vp, ep, up], dim=-1), it, cfg["output_mlp"])
    assert next(it, None) is None, "weights left over"
    return out


# ------------------------------------------------------------------------------------------------ named graph cases
MULTI_EDGES = [5, 0, 27, 1, 0, 40, 0, 3]
MULTI_NODES = [3, 2, 4, 1, 0, 5, 2, 2]


def _splits(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def hand_case(num_edges, seed=0):
    """One graph of 4 nodes where node 2 has no edges: receivers sorted, any sender.  ``(edge_indices, node_splits,
    edge_splits)`` with per-graph indices."""
    rng = np.random.default_rng(seed)
    recv = np.sort(rng.choice(np.array([0, 1, 3]), size=num_edges))
    idx = np.stack([recv, rng.integers(0, 4, size=num_edges)], axis=1).astype(np.int64).reshape(-1, 2)
    return idx, _splits([4]), _splits([num_edges])


def multi_case(seed=0, shuffled=False, graphs=len(MULTI_EDGES)):
    """Eight graphs (or the first ``graphs`` of them) with ``MULTI_EDGES`` edges and ``MULTI_NODES`` nodes: tile 0 of 32
    edges holds graphs 0 and 2 around an edgeless graph, graph 2 ends on the tile edge at 32, graph 5 crosses the edge at
    64, graph 4 has neither nodes nor edges, graphs 1 and 6 have nodes but no edges.  Receivers are sorted within each
    graph, senders are anywhere in it; ``shuffled`` permutes every graph's list."""
    rng = np.random.default_rng(seed)
    idx = []
    for e, n in zip(MULTI_EDGES[:graphs], MULTI_NODES[:graphs]):
        if e == 0:
            continue
        part = np.stack([np.sort(rng.integers(0, n, size=e)), rng.integers(0, n, size=e)], axis=1).astype(np.int64)
        if shuffled:
            part = part[rng.permutation(e)]
        idx.append(part)
    return np.concatenate(idx, axis=0), _splits(MULTI_NODES[:graphs]), _splits(MULTI_EDGES[:graphs])


def many_graphs_case(graphs=2100):
    """``graphs`` one-node graphs with 1, 0, 2, 1, 0, 2, ... self edges (the last one has edges): more graphs than
    csrc/mp_megnet.hip keeps row splits for in LDS (2048), so the graph of an edge is searched in global memory."""
    counts = np.array([1, 0, 2] * (graphs // 3 + 1))[:graphs]
    counts[-1] = 1
    return np.zeros((int(counts.sum()), 2), np.int64), _splits(np.ones(graphs, np.int64)), _splits(counts)
