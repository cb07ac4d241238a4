"""Differentiable torch-CPU restatement of the GAT family (kgcnn/layers/conv/gat_conv.py:103-114, 200-214, 233-323,
kgcnn/layers/pooling.py:464-546, kgcnn/ops/segment.py:5-24, kgcnn/literature/GAT.py:89-112), in float64 or float32: the
budget and the float32 twin of the GPU tests.  TEST INFRASTRUCTURE: no engine imports.

Written from the reference's op sequence: both end nodes are gathered, concatenated with the edge features, the Dense
layers run on the concatenation, the logits go through the segment softmax (segment maximum subtracted) and weight the
gathered messages in a segment sum.  Parameters are dictionaries with the keys of ``oracle.kgcnn_oracle``
(``linear_trafo/kernel``, ``alpha_activation/kernel``, ``alpha/kernel``, ``block{i}/head{h}/...``, ``dense0/...``,
``output_mlp/{k}/...``); ``idx`` is the flat ``(M, 2)`` int64 ``[receiver, sender]`` list of the whole batch.
"""
import numpy as np
import torch

ACTIVATIONS = {
    None: lambda x: x, "linear": lambda x: x, "relu": torch.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid,
    "softplus": torch.nn.functional.softplus, "swish": lambda x: x * torch.sigmoid(x),
    "kgcnn>leaky_relu": lambda x: torch.where(x >= 0, x, 0.05 * x),      # kgcnn/ops/activ.py: alpha = 0.05
    "leaky_relu": lambda x: torch.where(x >= 0, x, 0.05 * x),
}


def _t(a, dtype):
    if a is None:
        return None
    return a.to(dtype) if torch.is_tensor(a) else torch.tensor(np.asarray(a), dtype=dtype)


def params_to(p, dtype, requires_grad=False):
    """The parameter dictionary as torch leaves of ``dtype``."""
    return {k: _t(v, dtype).clone().requires_grad_(requires_grad) for k, v in p.items()}


def dense(x, kernel, bias, activation):
    y = x @ kernel
    if bias is not None:
        y = y + bias
    return ACTIVATIONS[activation](y)


def segment_softmax(logits, seg, rows):
    """kgcnn/ops/segment.py:5-24 with ``normalize=True`` on ``(M, C)`` logits."""
    if logits.shape[0] == 0:
        return logits
    index = seg[:, None].expand_as(logits)
    mx = torch.full((rows, logits.shape[1]), -np.inf, dtype=logits.dtype).scatter_reduce(0, index, logits.detach(), "amax")
    ex = torch.exp(logits - mx[seg])
    den = torch.zeros((rows, logits.shape[1]), dtype=logits.dtype).index_add(0, seg, ex)
    return ex / den[seg]


def attention_pool(messages, logits, recv, rows):
    """``PoolingLocalEdgesAttention`` (kgcnn/layers/pooling.py:464-546): a receiver without edges gets zeros."""
    w = segment_softmax(logits, recv, rows)
    return torch.zeros((rows, messages.shape[1]), dtype=messages.dtype).index_add(0, recv, w * messages)


def head(node, edge, idx, p, v2, act="kgcnn>leaky_relu", use_edge_features=False, use_final_activation=True,
         linear_activation="linear"):
    """One attention head -> ``(out (N, U), logits (M, 1))``.  ``linear_activation``: the activation of the message
    transform (``MultiHeadGATV2Layer`` gives it the head's activation, gat_conv.py:257)."""
    idx = torch.as_tensor(np.asarray(idx), dtype=torch.int64).reshape(-1, 2)
    recv, send = idx[:, 0], idx[:, 1]
    w_n = dense(node, p["linear_trafo/kernel"], p.get("linear_trafo/bias"), linear_activation)
    if v2:
        parts = [node[recv], node[send]] + ([edge] if use_edge_features else [])
        hidden = dense(torch.cat(parts, dim=-1), p["alpha_activation/kernel"], p.get("alpha_activation/bias"), act)
        logits = hidden @ p["alpha/kernel"]
    else:
        parts = [w_n[recv], w_n[send]] + ([edge] if use_edge_features else [])
        logits = dense(torch.cat(parts, dim=-1), p["alpha/kernel"], None, act)
    out = attention_pool(w_n[send], logits, recv, node.shape[0])
    if use_final_activation:
        out = ACTIVATIONS[act](out)
    return out, logits


def sub(params, prefix):
    return {k[len(prefix):]: v for k, v in params.items() if k.startswith(prefix)}


def multi_head(node, edge, idx, heads, act="kgcnn>leaky_relu", concat=True, use_edge_features=False,
               use_final_activation=True):
    """``MultiHeadGATV2Layer`` (gat_conv.py:233-323) -> ``(embeddings, logits (M, H, 1))``; ``heads``: one parameter
    dictionary per head."""
    outs, logits = zip(*[head(node, edge, idx, p, True, act, use_edge_features, use_final_activation, act) for p in heads])
    h = torch.cat(outs, dim=-1) if concat else sum(outs[1:], outs[0]) / len(outs)
    return h, torch.stack(logits, dim=1)


def model_forward(params, node_attr, edge_attr, idx, node_splits, depth=3, heads=5, concat=False, v2=False,
                  act="kgcnn>leaky_relu", use_edge_features=True, use_final_activation=False, pooling_method="mean",
                  output_mlp_act=("relu", "relu", "sigmoid"), output_mlp_bias=(True, True, False)):
    """``GAT.make_model`` / ``GATv2.make_model`` with ``output_embedding='graph'`` (kgcnn/literature/GAT.py:89-112).
    Integer ``node_attr`` / ``edge_attr`` (embedding inputs) index ``params['embed_n']`` / ``params['embed_e']``."""
    if not torch.is_floating_point(node_attr):
        node_attr = params["embed_n"][node_attr.reshape(-1)]
    if not torch.is_floating_point(edge_attr):
        edge_attr = params["embed_e"][edge_attr.reshape(-1)]
    nk = dense(node_attr, params["dense0/kernel"], params.get("dense0/bias"), "linear")
    for i in range(depth):
        outs = [head(nk, edge_attr, idx, sub(params, "block%d/head%d/" % (i, h)), v2, act, use_edge_features,
                     use_final_activation)[0] for h in range(heads)]
        if concat:
            nk = torch.cat(outs, dim=-1)
        else:
            nk = ACTIVATIONS[act](sum(outs[1:], outs[0]) / len(outs))
    s = np.asarray(node_splits, np.int64)
    graph = torch.from_numpy(np.repeat(np.arange(len(s) - 1), s[1:] - s[:-1]))
    pooled = torch.zeros((len(s) - 1, nk.shape[1]), dtype=nk.dtype).index_add(0, graph, nk)
    if pooling_method == "mean":
        pooled = pooled / torch.clamp(torch.from_numpy((s[1:] - s[:-1]).astype(np.float64)).to(nk.dtype), min=1.0)[:, None]
    for k, a in enumerate(output_mlp_act):
        pooled = dense(pooled, params["output_mlp/%d/kernel" % k],
                       params.get("output_mlp/%d/bias" % k) if output_mlp_bias[k] else None, a)
    return pooled


# ----------------------------------------------------------------------------------------------- parameters and cases
def glorot(rng, fan_in, fan_out):
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-lim, lim, size=(fan_in, fan_out)).astype(np.float32)


def head_params(rng, f, u, d, v2, bias=True, scale=1.0):
    """Glorot kernels and biases in +-0.1 of one head over ``f`` node and ``d`` edge features (``d = 0``: none)."""
    small = lambda n: rng.uniform(-0.1, 0.1, size=n).astype(np.float32)
    p = {"linear_trafo/kernel": glorot(rng, f, u)}
    if bias:
        p["linear_trafo/bias"] = small(u)
    if v2:
        p["alpha_activation/kernel"] = glorot(rng, 2 * f + d, u) * np.float32(scale)
        if bias:
            p["alpha_activation/bias"] = small(u)
        p["alpha/kernel"] = glorot(rng, u, 1)
    else:
        p["alpha/kernel"] = glorot(rng, 2 * u + d, 1) * np.float32(scale)
    return p


def model_params(rng, fn, fe, units, heads, depth, concat, v2, embed=None):
    """Parameters of ``model_forward`` in ``model.weights`` order (the dictionary's insertion order, after the two
    embedding tables, which the builder always owns).  ``embed = (node rows, edge rows)``: embedding inputs of widths
    ``fn`` / ``fe``."""
    p = {}
    if embed is not None:
        p["embed_n"] = rng.uniform(-0.5, 0.5, size=(embed[0], fn)).astype(np.float32)
        p["embed_e"] = rng.uniform(-0.5, 0.5, size=(embed[1], fe)).astype(np.float32)
    p["dense0/kernel"] = glorot(rng, fn, units)
    p["dense0/bias"] = rng.uniform(-0.1, 0.1, size=units).astype(np.float32)
    width = units
    for i in range(depth):
        for h in range(heads):
            for k, v in head_params(rng, width, units, fe, v2).items():
                p["block%d/head%d/%s" % (i, h, k)] = v
        width = units * heads if concat else units
    for k, (fin, fout, has_bias) in enumerate(((width, 25, True), (25, 10, True), (10, 1, False))):
        p["output_mlp/%d/kernel" % k] = glorot(rng, fin, fout)
        if has_bias:
            p["output_mlp/%d/bias" % k] = rng.uniform(-0.1, 0.1, size=fout).astype(np.float32)
    return p


# ----------------------------------------------------------------------------------------------- kernel cases
def kernel_cases():
    """name -> keyword arguments of ``kernel_case`` for every case tests/test_gpu_gat.py runs through the C ABI (both
    modes each).  Hub lists carry self loops and duplicate edges; their first and last node receive nothing."""
    import topologies as topo
    out = {
        "hub-sorted-u32-h5-d64": dict(order="sorted", u=32, h=5, d=64, f=32),
        "hub-shuffled-u64-h8-d3-f160": dict(order="shuffled", u=64, h=8, d=3, f=160),
        "hub-shuffled-u32-h1-d0-relu-nobias": dict(order="shuffled", u=32, h=1, d=0, f=32, act="relu", bias=False),
        "hub-sorted-u64-h5-d5-tanh": dict(order="sorted", u=64, h=5, d=5, f=32, act="tanh"),
        "hub-sorted-u32-h8-d1-tanh-nobias": dict(order="sorted", u=32, h=8, d=1, f=40, act="tanh", bias=False),
        "hub-shuffled-u64-h1-d64-relu": dict(order="shuffled", u=64, h=1, d=64, f=32, act="relu"),
        "x40-hub-shuffled-u32-h5-d64": dict(order="shuffled", u=32, h=5, d=64, f=32, scale=40.0),
        "x40-hub-sorted-u64-h5-d3-f160": dict(order="sorted", u=64, h=5, d=3, f=160, scale=40.0),
        "x40-hub-shuffled-u32-h5-d0": dict(order="shuffled", u=32, h=5, d=0, f=32, scale=40.0),
    }
    for total in topo.TILE_EXACT_SIZES:
        out["exact%d-u32-h5-d3" % total] = dict(kind="exact%d" % total, u=32, h=5, d=3, f=32)
    return out


def kernel_case(v2, kind="hub", order="sorted", u=32, h=5, d=64, f=32, act="kgcnn>leaky_relu", bias=True, scale=1.0,
                seed=0):
    """Inputs and weights of one attention block: ``nodes`` (N, f), ``edges`` (M, d), ``h`` heads of ``u`` units; the
    logit kernels scaled by ``scale`` (x40: logits of a few hundred, which overflow a softmax without the maximum)."""
    import topologies as topo
    if kind == "hub":
        graphs = topo.with_empty_graphs([(1100, topo.hub_edges(1100, topo.STANDARD_DEGREES, seed, True, True, order)),
                                         (60, topo.hub_edges(60, (2, 96, 5), seed + 1, True, True, order))])
    else:
        graphs = [topo.tile_exact(int(kind[5:]), seed=seed)]
    b = topo.batch(graphs)
    rng = np.random.default_rng(3000 + seed + 7 * u + d)
    n, m = int(b["row_splits"][-1]), len(b["flat"])
    b.update(nodes=rng.normal(size=(n, f)).astype(np.float32), edges=rng.normal(size=(m, d)).astype(np.float32),
             heads=[head_params(rng, f, u, d, v2, bias, scale) for _ in range(h)], v2=v2, act=act, u=u, d=d, rows=n)
    return b


def kernel_restate(case, dtype):
    """``(out (N, H, U), logits (M, H))`` of the case, numpy."""
    node, edge = _t(case["nodes"], dtype), _t(case["edges"], dtype)
    outs, logits = zip(*[head(node, edge, case["flat"], params_to(p, dtype), case["v2"], case["act"], case["d"] > 0,
                              False) for p in case["heads"]])
    return torch.stack(outs, dim=1).numpy(), torch.cat(logits, dim=-1).numpy()
