"""Differentiable torch-CPU restatement of AttentiveFP (kgcnn/layers/conv/attentivefp_conv.py:75-107, 196-220,
kgcnn/literature/AttentiveFP.py:102-122, the Keras GRUCell with ``reset_after=True``), in float64 or float32: the budget
and the float32 twin of the GPU tests.  TEST INFRASTRUCTURE: no engine imports.

Written from the reference's per-edge op order: both end nodes are gathered, the sender row is concatenated with the edge
features, the Dense layers run on the gathered rows and their concatenations, the logits go through the segment softmax
and weight the gathered messages in a segment sum; the readout repeats the graph state over the graph's nodes,
concatenates and runs the Dense layers per node.  Parameters are dictionaries (``linear_trafo/kernel``,
``alpha_activation/kernel``, ``alpha/kernel``, ``fc1/...``, ``fc2/...``, ``gru/kernel | recurrent_kernel | bias``,
``head{i}/...``, ``update{i}/...``, ``readout/...``, ``dense0/...``, ``output_mlp/{k}/...``); ``idx`` is the flat
``(M, 2)`` int64 ``[receiver, sender]`` list of the whole batch.
"""
import numpy as np
import torch

from gat_reference import ACTIVATIONS as _GAT_ACTIVATIONS
from gat_reference import _t, attention_pool, dense, glorot, params_to, segment_softmax, sub   # noqa: F401

ACTIVATIONS = dict(_GAT_ACTIVATIONS, elu=torch.nn.functional.elu)


def _dense(x, p, name, activation):
    y = x @ p[name + "/kernel"]
    if p.get(name + "/bias") is not None:
        y = y + p[name + "/bias"]
    return ACTIVATIONS[activation](y)


def head(node, edge, idx, p, use_edge_features, act="kgcnn>leaky_relu", act_context="elu"):
    """``AttentiveHeadFP.call`` -> ``(out (N, U), logits (M, 1))``."""
    idx = torch.as_tensor(np.asarray(idx), dtype=torch.int64).reshape(-1, 2)
    recv, send = idx[:, 0], idx[:, 1]
    n_in, n_out = node[recv], node[send]
    if use_edge_features:
        n_in = _dense(n_in, p, "fc1", act)
        n_out = _dense(torch.cat([n_out, edge], dim=-1), p, "fc2", act)
    wn_out = _dense(n_out, p, "linear_trafo", "linear")
    e_ij = _dense(torch.cat([n_in, n_out], dim=-1), p, "alpha_activation", act)
    logits = e_ij @ p["alpha/kernel"]
    out = attention_pool(wn_out, logits, recv, node.shape[0])
    return ACTIVATIONS[act_context](out), logits


def gru_cell(x, h, p, prefix="gru", act="tanh", rec_act="sigmoid"):
    """Keras GRUCell, ``reset_after=True``: gates ``[z | r | h]``, bias rows input / recurrent."""
    u = h.shape[1]
    mx, mh = x @ p[prefix + "/kernel"], h @ p[prefix + "/recurrent_kernel"]
    if p.get(prefix + "/bias") is not None:
        mx, mh = mx + p[prefix + "/bias"][0], mh + p[prefix + "/bias"][1]
    z = ACTIVATIONS[rec_act](mx[:, :u] + mh[:, :u])
    r = ACTIVATIONS[rec_act](mx[:, u:2 * u] + mh[:, u:2 * u])
    hh = ACTIVATIONS[act](mx[:, 2 * u:] + r * mh[:, 2 * u:])
    return z * h + (1.0 - z) * hh


def graph_rows(node_splits):
    """Rows ``PoolingNodes`` returns: trailing empty graphs are dropped."""
    s = np.asarray(node_splits, np.int64)
    rows = len(s) - 1
    while rows > 0 and s[rows] == s[rows - 1]:
        rows -= 1
    return rows


def readout(node, node_splits, p, depth=3, pooling_method="sum", act="kgcnn>leaky_relu", act_context="elu",
            rec_act="sigmoid"):
    """``PoolingNodesAttentive.call`` -> ``(rows, U)``."""
    s = np.asarray(node_splits, np.int64)
    rows = graph_rows(s)
    lens = s[1:rows + 1] - s[:rows]
    graph = torch.from_numpy(np.repeat(np.arange(rows), lens))
    h = torch.zeros((rows, node.shape[1]), dtype=node.dtype).index_add(0, graph, node)
    if pooling_method == "mean":
        h = h / torch.clamp(torch.from_numpy(lens.astype(np.float64)).to(node.dtype), min=1.0)[:, None]
    wn = _dense(node, p, "linear_trafo", "linear")
    for _ in range(depth):
        av = _dense(torch.cat([h[graph], node], dim=-1), p, "alpha", act)
        cont = ACTIVATIONS[act_context](attention_pool(wn, av, graph, rows))
        h = gru_cell(cont, h, p, rec_act=rec_act)
    return h


def model_forward(params, node_attr, edge_attr, idx, node_splits, depthato=2, depthmol=2, output_embedding="graph",
                  output_mlp_act=("relu", "relu", "sigmoid"), output_mlp_bias=(True, True, False)):
    """``AttentiveFP.make_model`` (kgcnn/literature/AttentiveFP.py:96-122).  Integer ``node_attr`` / ``edge_attr``
    (embedding inputs) index ``params['embed_n']`` / ``params['embed_e']``.  Node output: ``(N, L)`` flat rows."""
    if not torch.is_floating_point(node_attr):
        node_attr = params["embed_n"][node_attr.reshape(-1)]
    if not torch.is_floating_point(edge_attr):
        edge_attr = params["embed_e"][edge_attr.reshape(-1)]
    nk = _dense(node_attr, params, "dense0", "linear")
    for i in range(max(depthato, 1)):
        ck = head(nk, edge_attr, idx, sub(params, "head%d/" % i), i == 0)[0]
        nk = gru_cell(ck, nk, sub(params, "update%d/" % i))
    out = readout(nk, node_splits, sub(params, "readout/"), depth=depthmol) if output_embedding == "graph" else nk
    for k, a in enumerate(output_mlp_act):
        out = dense(out, params["output_mlp/%d/kernel" % k],
                    params.get("output_mlp/%d/bias" % k) if output_mlp_bias[k] else None, a)
    return out


# ----------------------------------------------------------------------------------------------- parameters
def _small(rng, n):
    return rng.uniform(-0.1, 0.1, size=n).astype(np.float32)


def head_params(rng, f, u, d, bias=True, scale=1.0):
    """One head over ``f`` node features; ``d > 0``: with edge features of that width.  Insertion order = the layer's
    ``weights`` order.  ``scale`` multiplies the hidden logit kernel (x40: logits of tens to hundreds)."""
    w = f if d == 0 else u
    p = {"linear_trafo/kernel": glorot(rng, w, u)}
    if bias:
        p["linear_trafo/bias"] = _small(rng, u)
    p["alpha_activation/kernel"] = glorot(rng, 2 * w, u) * np.float32(scale)
    if bias:
        p["alpha_activation/bias"] = _small(rng, u)
    p["alpha/kernel"] = glorot(rng, u, 1)
    if d > 0:
        for name, fan in (("fc1", f), ("fc2", f + d)):
            p[name + "/kernel"] = glorot(rng, fan, u)
            if bias:
                p[name + "/bias"] = _small(rng, u)
    return p


def gru_params(rng, fin, u, prefix="gru", bias=True):
    p = {prefix + "/kernel": glorot(rng, fin, 3 * u), prefix + "/recurrent_kernel": glorot(rng, u, 3 * u)}
    if bias:
        p[prefix + "/bias"] = rng.uniform(-0.1, 0.1, size=(2, 3 * u)).astype(np.float32)
    return p


def readout_params(rng, u, bias=True, scale=1.0):
    """Insertion order = ``PoolingNodesAttentive.weights``.  ``scale`` multiplies ``alpha/kernel`` (peaked softmax)."""
    p = {"linear_trafo/kernel": glorot(rng, u, u)}
    if bias:
        p["linear_trafo/bias"] = _small(rng, u)
    p["alpha/kernel"] = glorot(rng, 2 * u, 1) * np.float32(scale)
    if bias:
        p["alpha/bias"] = _small(rng, 1)
    p.update(gru_params(rng, u, u, bias=bias))
    return p


def model_params(rng, fn, fe, units, depthato=2, embed=None, output_embedding="graph"):
    """Parameters of ``model_forward`` in ``model.weights`` order.  ``embed = (node rows, edge rows)``: embedding inputs
    of widths ``fn`` / ``fe``."""
    p = {}
    if embed is not None:
        p["embed_n"] = rng.uniform(-0.5, 0.5, size=(embed[0], fn)).astype(np.float32)
        p["embed_e"] = rng.uniform(-0.5, 0.5, size=(embed[1], fe)).astype(np.float32)
    p["dense0/kernel"] = glorot(rng, fn, units)
    p["dense0/bias"] = _small(rng, units)
    for i in range(max(depthato, 1)):
        for k, v in head_params(rng, units, units, fe if i == 0 else 0).items():
            p["head%d/%s" % (i, k)] = v
        for k, v in gru_params(rng, units, units).items():
            p["update%d/%s" % (i, k)] = v
    if output_embedding == "graph":
        for k, v in readout_params(rng, units).items():
            p["readout/" + k] = v
    for k, (fin, fout, has_bias) in enumerate(((units, 25, True), (25, 10, True), (10, 1, False))):
        p["output_mlp/%d/kernel" % k] = glorot(rng, fin, fout)
        if has_bias:
            p["output_mlp/%d/bias" % k] = _small(rng, fout)
    return p


# ----------------------------------------------------------------------------------------------- edge-head kernel cases
HUB_DEGREES = (1, 63, 64, 65, 200)


def edge_cases():
    """name -> keyword arguments of ``edge_case`` for every case tests/test_gpu_attentivefp.py runs through the C ABI."""
    out = {
        "hub-sorted-u32-d5-f7": dict(order="sorted", u=32, d=5, f=7),
        "hub-shuffled-u64-d3-f64": dict(order="shuffled", u=64, d=3, f=64),
        "hub-shuffled-u32-d64-f64-relu-nobias": dict(order="shuffled", u=32, d=64, f=64, act="relu", bias=False),
        "hub-sorted-u64-d1-f7-tanh": dict(order="sorted", u=64, d=1, f=7, act="tanh", act_context="tanh"),
        "hub-sorted-u64-d64-f7-nobias": dict(order="sorted", u=64, d=64, f=7, bias=False, act_context="linear"),
        "x40-hub-shuffled-u32-d5-f64": dict(order="shuffled", u=32, d=5, f=64, scale=40.0),
        "x40-hub-sorted-u64-d3-f7": dict(order="sorted", u=64, d=3, f=7, scale=40.0),
    }
    for total in (0, 1, 31, 32, 33, 65):
        out["exact%d-u32-d3-f7" % total] = dict(kind="exact%d" % total, u=32, d=3, f=7)
    return out


def edge_case(kind="hub", order="sorted", u=32, d=5, f=7, act="kgcnn>leaky_relu", act_context="elu", bias=True, scale=1.0,
              seed=0):
    """Inputs and weights of one head with edge features: ``nodes`` (N, f), ``edges`` (M, d).  Hub lists carry self loops
    and duplicate edges, receivers of degree 1 / 63 / 64 / 65 / 200 in one list, their first and last node receive
    nothing, and empty graphs stand first, in the middle and last."""
    import topologies as topo
    if kind == "hub":
        graphs = topo.with_empty_graphs([(260, topo.hub_edges(260, HUB_DEGREES, seed, True, True, order)),
                                         (60, topo.hub_edges(60, (2, 96, 5), seed + 1, True, True, order))])
    else:
        graphs = [topo.tile_exact(int(kind[5:]), seed=seed)]
    b = topo.batch(graphs)
    rng = np.random.default_rng(5000 + seed + 7 * u + d)
    n, m = int(b["row_splits"][-1]), len(b["flat"])
    b.update(nodes=rng.normal(size=(n, f)).astype(np.float32), edges=rng.normal(size=(m, d)).astype(np.float32),
             params=head_params(rng, f, u, d, bias, scale), act=act, act_context=act_context, u=u, d=d, rows=n)
    return b


def edge_restate(case, dtype):
    """``(out (N, U), logits (M,))`` of the case in edge order, numpy."""
    out, logits = head(_t(case["nodes"], dtype), _t(case["edges"], dtype), case["flat"], params_to(case["params"], dtype),
                       True, case["act"], case["act_context"])
    return out.numpy(), logits.numpy().reshape(-1)


# ----------------------------------------------------------------------------------------------- readout kernel cases
TILE_LENGTHS = [0, 1, 2, 63, 64, 65, 300, 5, 0, 17, 3, 1, 40, 9, 2, 0]   # 16 graphs = one workgroup


def readout_cases():
    """name -> keyword arguments of ``readout_case``."""
    few = lambda g: [int(v) for v in 1 + (np.arange(g) * 7) % 11]
    out = {
        "tile-u32-d3-sum": dict(lengths=TILE_LENGTHS, u=32, depth=3),
        "tile-u36-d1-mean": dict(lengths=TILE_LENGTHS, u=36, depth=1, pooling_method="mean"),
        "tile-u64-d3-mean-peaked": dict(lengths=TILE_LENGTHS, u=64, depth=3, pooling_method="mean", scale=30.0),
        "tile-u200-d3-sum": dict(lengths=TILE_LENGTHS, u=200, depth=3),
        "tile-u200-d0-sum": dict(lengths=TILE_LENGTHS, u=200, depth=0),
        "tile-u32-d3-sum-peaked-nobias": dict(lengths=TILE_LENGTHS, u=32, depth=3, scale=30.0, bias=False),
        "empty-first-interior-last-u36-d3": dict(lengths=[0, 4, 0, 0, 7, 2, 0], u=36, depth=3),
    }
    for g in (1, 15, 16, 17, 33):
        out["g%d-u64-d1-sum" % g] = dict(lengths=few(g), u=64, depth=1)
    return out


def readout_case(lengths, u=32, depth=3, pooling_method="sum", scale=1.0, bias=True, act="kgcnn>leaky_relu",
                 act_context="elu", seed=0):
    """Node rows are 0.3 x normal: a sum over 300 of them stays O(5), so the GRU gates are not saturated."""
    rng = np.random.default_rng(7000 + seed + 3 * u + depth + len(lengths))
    splits = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return {"nodes": (0.3 * rng.normal(size=(int(splits[-1]), u))).astype(np.float32), "row_splits": splits,
            "params": readout_params(rng, u, bias, scale), "u": u, "depth": depth, "pooling_method": pooling_method,
            "act": act, "act_context": act_context}


def readout_restate(case, dtype):
    return readout(_t(case["nodes"], dtype), case["row_splits"], params_to(case["params"], dtype), case["depth"],
                   case["pooling_method"], case["act"], case["act_context"]).numpy()
