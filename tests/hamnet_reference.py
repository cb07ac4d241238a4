"""Differentiable torch-CPU restatement of HamNet (kgcnn/layers/conv/hamnet_conv.py:85-88, 194-207, 358-368, 508-528,
kgcnn/literature/HamNet.py:107-164, the Keras GRUCell with ``reset_after=True``), in float64 or float32: the budget and the
float32 twin of the GPU tests, and the builders of their cases.  TEST INFRASTRUCTURE: no engine imports.

Written from the reference's op order in concatenated form: both end nodes' features, momenta and coordinates are
gathered per edge, the differences are taken on the gathered rows, ``[p_uv || q_uv || he]`` and ``[h_u || p_uv || q_uv ||
h_v]`` are concatenated and go through ONE Dense each, the attend Dense runs on the gathered sender rows; the readout
repeats the graph state over the graph's nodes, concatenates ``[s || h]`` and runs the Dense per node.  None of the
kernels' algebraic splits (node-side products, row blocks of a kernel) appears here.  Parameters are dictionaries whose
insertion order is the layers' ``weights`` order; ``idx`` is the flat ``(M, 2)`` int64 ``[receiver, sender]`` list of the
whole batch.
"""
import numpy as np
import torch

from attentivefp_reference import ACTIVATIONS, graph_rows, gru_cell
from gat_reference import _t, attention_pool, dense, glorot, params_to, sub   # noqa: F401

LEAKY, ELU = "kgcnn>leaky_relu", "elu"


def _dense(x, p, name, activation):
    y = x @ p[name + "/kernel"]
    if p.get(name + "/bias") is not None:
        y = y + p[name + "/bias"]
    return ACTIVATIONS[activation](y)


# ----------------------------------------------------------------------------------------------- layers
def message(h, he, pm, q, idx, p, act=LEAKY, act_last=ELU, edge_update=True):
    """``HamNaiveDynMessage.call`` -> ``(mv (N, U), me (M, UE) or None, logits (M, 1))``."""
    idx = torch.as_tensor(np.asarray(idx), dtype=torch.int64).reshape(-1, 2)
    u, v = idx[:, 0], idx[:, 1]
    h_u, h_v = h[u], h[v]
    p_uv, q_uv = pm[v] - pm[u], q[v] - q[u]
    attend = _dense(h_v, p, "attend", act)
    align = _dense(torch.cat([p_uv, q_uv, he], dim=-1), p, "align", "linear")
    mv = ACTIVATIONS[act_last](attention_pool(attend, align, u, h.shape[0]))
    me = _dense(torch.cat([h_u, p_uv, q_uv, h_v], dim=-1), p, "edge", act) if edge_update else None
    return mv, me, align


def naive_union(x, xu, p, act=LEAKY):
    """``HamNetNaiveUnion.call``."""
    return _dense(torch.cat([x, xu], dim=-1), p, "dense", act)


def readout_attend(s, h, graph, rows, p, act=LEAKY, act_last=ELU):
    """``HamNetGlobalReadoutAttend.call`` -> ``(m (rows, UA), a (n, 1))``; ``graph``: the graph of every node."""
    attend = _dense(h, p, "attend", act)
    align = _dense(torch.cat([s[graph], h], dim=-1), p, "align", "linear")
    return ACTIVATIONS[act_last](attention_pool(attend, align, graph, rows)), align


def fingerprint(h, node_splits, p, depth, pooling_method="mean", act=LEAKY, rows=None):
    """``HamNetFingerprintGenerator.call`` -> ``(rows, U)``; ``rows``: the graphs to return (default: ``PoolingNodes``'
    count, the trailing empty graphs dropped; the kernel itself serves every graph it is given)."""
    s = np.asarray(node_splits, np.int64)
    rows = graph_rows(s) if rows is None else rows
    lens = s[1:rows + 1] - s[:rows]
    graph = torch.from_numpy(np.repeat(np.arange(rows), lens))
    m = _dense(h, p, "v2m", act)
    state = torch.zeros((rows, m.shape[1]), dtype=h.dtype).index_add(0, graph, m[:len(graph)])
    if pooling_method == "mean":
        state = state / torch.clamp(torch.from_numpy(lens.astype(np.float64)).to(h.dtype), min=1.0)[:, None]
    for i in range(depth):
        mm, _ = readout_attend(state, h[:len(graph)], graph, rows, sub(p, "r%d/" % i), act)
        state = ACTIVATIONS[act](gru_cell(mm, state, p, prefix="g%d" % i))
    return state


def _unite(kind, x, xu, p, prefix):
    if kind == "gru":
        return gru_cell(xu, x, p, prefix=prefix + "/gru")
    if kind == "naive":
        return naive_union(x, xu, sub(p, prefix + "/"))
    return xu


def model_forward(params, node_attr, edge_attr, idx, coords, node_splits, depth=1, fp_depth=2, union_node="gru",
                  union_edge="None", output_embedding="graph", output_mlp_act=("relu", "relu", "linear"),
                  output_mlp_bias=(True, True, False)):
    """``HamNet.make_model`` (kgcnn/literature/HamNet.py:107-164).  Integer ``node_attr`` / ``edge_attr`` (embedding
    inputs) index ``params['embed_n']`` / ``params['embed_e']``.  Node output: ``(N, L)`` flat rows."""
    if not torch.is_floating_point(node_attr):
        node_attr = params["embed_n"][node_attr.reshape(-1)]
    if not torch.is_floating_point(edge_attr):
        edge_attr = params["embed_e"][edge_attr.reshape(-1)]
    n = _dense(node_attr, params, "dense_n", "tanh")
    ed = _dense(edge_attr, params, "dense_e", "tanh")
    q, pm = coords, torch.zeros_like(coords)
    for i in range(depth):
        nu, eu, _ = message(n, ed, pm, q, idx, sub(params, "msg%d/" % i))
        n = _unite(union_node, n, nu, params, "nu%d" % i)
        ed = _unite(union_edge, ed, eu, params, "eu%d" % i)
    out = fingerprint(n, node_splits, sub(params, "fp/"), fp_depth) if output_embedding == "graph" else n
    for k, a in enumerate(output_mlp_act):
        out = dense(out, params["output_mlp/%d/kernel" % k],
                    params.get("output_mlp/%d/bias" % k) if output_mlp_bias[k] else None, a)
    return out


# ----------------------------------------------------------------------------------------------- parameters
def _small(rng, n):
    return rng.uniform(-0.1, 0.1, size=n).astype(np.float32)


def _dense_params(p, rng, name, fin, fout, bias):
    p[name + "/kernel"] = glorot(rng, fin, fout)
    if bias:
        p[name + "/bias"] = _small(rng, fout)


def message_params(rng, f, d, c, u, ue, bias=True):
    """Insertion order = ``HamNaiveDynMessage.weights``."""
    p = {}
    _dense_params(p, rng, "attend", f, u, bias)
    _dense_params(p, rng, "align", 2 * c + d, 1, bias)
    _dense_params(p, rng, "edge", 2 * f + 2 * c, ue, bias)
    return p


def gru_params(rng, fin, u, prefix, bias=True):
    p = {prefix + "/kernel": glorot(rng, fin, 3 * u), prefix + "/recurrent_kernel": glorot(rng, u, 3 * u)}
    if bias:
        p[prefix + "/bias"] = rng.uniform(-0.1, 0.1, size=(2, 3 * u)).astype(np.float32)
    return p


def fingerprint_params(rng, f, u, ua, depth, bias=True, scale=1.0):
    """Insertion order = ``HamNetFingerprintGenerator.weights``.  ``scale`` multiplies the align kernels (peaked softmax)."""
    p = {}
    _dense_params(p, rng, "v2m", f, u, bias)
    for i in range(depth):
        _dense_params(p, rng, "r%d/attend" % i, f, ua, bias)
        _dense_params(p, rng, "r%d/align" % i, u + f, 1, bias)
        p["r%d/align/kernel" % i] = p["r%d/align/kernel" % i] * np.float32(scale)
        p.update(gru_params(rng, ua, u, "g%d" % i, bias))
    return p


def _union_params(p, rng, kind, prefix, fx, fu, units):
    if kind == "gru":
        p.update(gru_params(rng, fu, units, prefix + "/gru"))
    elif kind == "naive":
        _dense_params(p, rng, prefix + "/dense", fx + fu, units, True)


def model_params(rng, fn, fe, units=128, depth=1, fp_depth=2, union_node="gru", union_edge="None", embed=(95, 5),
                 coords=3, output_embedding="graph"):
    """Parameters of ``model_forward`` in ``model.weights`` order (message, node union, edge union per round)."""
    p = {}
    if embed is not None:
        p["embed_n"] = rng.uniform(-0.5, 0.5, size=(embed[0], fn)).astype(np.float32)
        p["embed_e"] = rng.uniform(-0.5, 0.5, size=(embed[1], fe)).astype(np.float32)
    _dense_params(p, rng, "dense_n", fn, units, True)
    _dense_params(p, rng, "dense_e", fe, units, True)
    nw = ew = units
    for i in range(depth):
        for k, v in message_params(rng, nw, ew, coords, units, units).items():
            p["msg%d/%s" % (i, k)] = v
        _union_params(p, rng, union_node, "nu%d" % i, nw, units, units)
        _union_params(p, rng, union_edge, "eu%d" % i, ew, units, units)
        nw = ew = units
    if output_embedding == "graph":
        for k, v in fingerprint_params(rng, nw, units, units, fp_depth).items():
            p["fp/" + k] = v
    # The output MLP ends in a linear Dense without bias.  With signed kernels an output row is a difference of hidden
    # terms fifty times its size, and a row-wise comparison of two float32 pipelines then measures that cancellation
    # (the float32 restatement itself sits 4e-5 from float64 there).  Non-negative kernels and biases behind the first
    # ReLU keep every row at the scale of what it sums.
    for k, (fin, fout, has_bias) in enumerate(((units, 25, True), (25, 10, True), (10, 1, False))):
        kernel = glorot(rng, fin, fout)
        p["output_mlp/%d/kernel" % k] = kernel if k == 0 else np.abs(kernel)
        if has_bias:
            p["output_mlp/%d/bias" % k] = np.abs(_small(rng, fout))
    return p


# ----------------------------------------------------------------------------------------------- message kernel cases
HUB_DEGREES = (1, 63, 64, 65, 130)   # beside the receivers of in-degree 0: across the 64-position chunk and the wave
LOGIT_REACH = 90.0                   # "x80" cases: float32 exp overflows above 88.7, so the segment maximum has to go first


def message_cases():
    """name -> keyword arguments of ``message_case`` for every case tests/test_gpu_hamnet.py runs through the C ABI."""
    return {
        "hub-sorted-f4-u4-ue4-d4-c1": dict(order="sorted", f=4, u=4, ue=4, d=4, c=1),
        "hub-shuffled-f12-u36-ue20-d12-c3": dict(order="shuffled", f=12, u=36, ue=20, d=12),
        "hub-sorted-f12-u36-ue20-d20-c3-nobias": dict(order="sorted", f=12, u=36, ue=20, d=20, bias=False),
        "hub-sorted-f128-u128-ue128-d128-c3": dict(order="sorted", f=128, u=128, ue=128, d=128),
        "hub-shuffled-f256-u256-ue256-d256-c8": dict(order="shuffled", f=256, u=256, ue=256, d=256, c=8),
        "hub-shuffled-f12-u36-ue20-d36-c8-tanh": dict(order="shuffled", f=12, u=36, ue=20, d=36, c=8, act="tanh",
                                                     act_last="linear"),
        "x80-hub-shuffled-f12-u36-ue20-d12-c3": dict(order="shuffled", f=12, u=36, ue=20, d=12, reach=LOGIT_REACH),
        "far-hub-sorted-f12-u36-ue20-d12-c3": dict(order="sorted", f=12, u=36, ue=20, d=12, offset=1e3),
        "noedges-f12-u36-ue20-d12-c3": dict(kind="noedges", f=12, u=36, ue=20, d=12),
    }


def message_case(kind="hub", order="sorted", f=12, u=36, ue=20, d=12, c=3, act=LEAKY, act_last=ELU, bias=True, reach=None,
                 offset=0.0, seed=0):
    """Inputs and weights of one message step: ``nodes`` (N, f), ``edges`` (M, d), ``p``, ``q`` (N, c).  Hub lists carry
    self loops and duplicate edges, receivers of in-degree 0 / 1 / 63 / 64 / 65 / 130 in one list, and empty graphs stand
    first, in the middle and last.  ``reach``: the edge rows are scaled so that the largest logit is about that far from
    zero; ``offset`` moves every coordinate and momentum away from the origin."""
    import topologies as topo
    if kind == "hub":
        graphs = topo.with_empty_graphs([(270, topo.hub_edges(270, HUB_DEGREES, seed, True, True, order)),
                                         (60, topo.hub_edges(60, (2, 96, 5), seed + 1, True, True, order))])
    else:
        graphs = [(5, np.zeros((0, 2), np.int64)), (0, np.zeros((0, 2), np.int64))]
    b = topo.batch(graphs)
    rng = np.random.default_rng(9000 + seed + 7 * u + d + 3 * c)
    n, m = int(b["row_splits"][-1]), len(b["flat"])
    params = message_params(rng, f, d, c, u, ue, bias)
    edges = rng.normal(size=(m, d)).astype(np.float32)
    if reach is not None and m:
        plain = np.abs(edges.astype(np.float64) @ params["align/kernel"][2 * c:].astype(np.float64)).max()
        edges = (edges * np.float32(reach / plain)).astype(np.float32)
    b.update(nodes=rng.normal(size=(n, f)).astype(np.float32), edges=edges,
             p=(rng.normal(size=(n, c)) + offset).astype(np.float32), q=(rng.normal(size=(n, c)) + offset).astype(np.float32),
             params=params, act=act, act_last=act_last, f=f, u=u, ue=ue, d=d, c=c, rows=n)
    return b


def message_restate(case, dtype):
    """``(mv (N, U), me (M, UE), logits (M,))`` of the case in edge order, numpy."""
    mv, me, logits = message(_t(case["nodes"], dtype), _t(case["edges"], dtype), _t(case["p"], dtype),
                             _t(case["q"], dtype), case["flat"], params_to(case["params"], dtype), case["act"],
                             case["act_last"])
    return mv.numpy(), me.numpy(), logits.numpy().reshape(-1)


# ----------------------------------------------------------------------------------------------- fingerprint kernel cases
TILE_LENGTHS = [1, 64, 0, 65, 130, 5, 0, 17, 3, 1, 40, 9, 2, 2, 0, 0]   # 16 graphs = one workgroup, two trailing empties


def fingerprint_cases():
    """name -> keyword arguments of ``fingerprint_case``."""
    few = lambda g: [int(v) for v in 1 + (np.arange(g) * 7) % 11]
    out = {
        "tile-f12-u8-ua20-d4-mean": dict(lengths=TILE_LENGTHS, depth=4),
        "tile-f12-u8-ua20-d8-sum-nobias": dict(lengths=TILE_LENGTHS, depth=8, pooling_method="sum", bias=False),
        "tile-f12-u8-ua20-d0-mean": dict(lengths=TILE_LENGTHS, depth=0),
        "tile-f128-u128-ua128-d1-sum": dict(lengths=TILE_LENGTHS, f=128, u=128, ua=128, depth=1, pooling_method="sum"),
        "tile-f128-u128-ua128-d4-mean-peaked": dict(lengths=TILE_LENGTHS, f=128, u=128, ua=128, depth=4, scale=30.0),
        "empty-first-interior-last-f12-u8-ua20-d4": dict(lengths=[0, 4, 0, 0, 7, 2, 0], depth=4),
    }
    for g in (1, 16, 17, 33):
        out["g%d-f12-u8-ua20-d1-mean" % g] = dict(lengths=few(g), depth=1)
    return out


def fingerprint_case(lengths, f=12, u=8, ua=20, depth=4, pooling_method="mean", scale=1.0, bias=True, act=LEAKY, seed=0):
    """Node rows are 0.3 x normal: a sum over 130 of them stays O(3), so the GRU gates are not saturated."""
    rng = np.random.default_rng(11000 + seed + 3 * u + depth + len(lengths))
    splits = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return {"nodes": (0.3 * rng.normal(size=(int(splits[-1]), f))).astype(np.float32), "row_splits": splits,
            "params": fingerprint_params(rng, f, u, ua, depth, bias, scale), "f": f, "u": u, "ua": ua, "depth": depth,
            "pooling_method": pooling_method, "act": act, "bias": bias}


def fingerprint_restate(case, dtype, rows=None):
    return fingerprint(_t(case["nodes"], dtype), case["row_splits"], params_to(case["params"], dtype), case["depth"],
                       case["pooling_method"], case["act"], rows=rows).numpy()


# ----------------------------------------------------------------------------------------------- molecule-like batches
MOL_SIZES = (9, 5, 12, 1, 7, 0, 14, 3, 6, 8, 2, 11, 4, 10, 5, 7, 13, 6, 9)   # 19 graphs, one of them empty


def mol_batch(sizes=MOL_SIZES, seed=3, fn=12, fe=8, coords=3, embed=False):
    """Bond graphs of these sizes (a random tree plus two ring bonds, both directions, sorted by receiver and sender);
    ``x`` / ``e``: float features, or float32 type numbers for the embedding inputs; ``xyz``: coordinates."""
    import topologies as topo
    rng = np.random.default_rng(seed)
    graphs = []
    for n in sizes:
        bonds = {(int(rng.integers(0, a)), a) for a in range(1, n)}
        for _ in range(2 if n > 3 else 0):
            a, b = (int(v) for v in rng.choice(n, size=2, replace=False))
            bonds.add((min(a, b), max(a, b)))
        directed = sorted([(a, b) for a, b in bonds] + [(b, a) for a, b in bonds])
        graphs.append((n, np.array(directed, dtype=np.int64).reshape(-1, 2)))
    b = topo.batch(graphs)
    n, m = int(b["row_splits"][-1]), len(b["flat"])
    if embed:
        b["x"], b["e"] = rng.integers(0, 95, size=n).astype(np.float32), rng.integers(0, 5, size=m).astype(np.float32)
    else:
        b["x"], b["e"] = rng.normal(size=(n, fn)).astype(np.float32), rng.normal(size=(m, fe)).astype(np.float32)
    b["xyz"] = (1.5 * rng.normal(size=(n, coords))).astype(np.float32)
    b["embedded"], b["sizes"] = embed, tuple(sizes)
    return b
