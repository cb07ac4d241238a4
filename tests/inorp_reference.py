"""Torch restatement of INorp (kgcnn/literature/INorp.py:99-153) for the tests, in any dtype (float32 with its float64
twin as budget): one block's edge step as a per-edge loop, in tensor form and folded (the form csrc/mp_inorp.hip
computes), the closed forms of the folded step's reverse, and the whole model on the weights in the model's order.  Also
the hand-made edge lists, the model configurations and the weight draws the CPU and GPU tests share.  No engine import."""
import numpy as np
import torch

ALPHA = 0.05
_SELU_SCALE, _SELU_ALPHA = 1.0507009873554805, 1.6732632423543772
LN2 = 0.6931471805599453

ACTIVATIONS = ["linear", "relu", "kgcnn>shifted_softplus", "softplus", "swish", "sigmoid", "tanh", "kgcnn>leaky_relu",
               "kgcnn>softplus2", "selu"]          # the engine's codes 0..9 (include/mpengine/core.h)


def act(name, x):
    name = (name or "linear").replace("kgcnn>", "")
    if name == "linear":
        return x
    if name == "relu":
        return torch.relu(x)
    if name == "shifted_softplus":
        return torch.nn.functional.softplus(x) - LN2
    if name == "softplus":
        return torch.nn.functional.softplus(x)
    if name == "swish":
        return x * torch.sigmoid(x)
    if name == "sigmoid":
        return torch.sigmoid(x)
    if name == "tanh":
        return torch.tanh(x)
    if name == "leaky_relu":
        return torch.where(x >= 0, x, ALPHA * x)
    if name == "softplus2":
        return torch.relu(x) + torch.log(0.5 * torch.exp(-torch.abs(x)) + 0.5)
    if name == "selu":
        return _SELU_SCALE * torch.where(x > 0, x, _SELU_ALPHA * (torch.exp(torch.clamp(x, max=0.0)) - 1.0))
    raise ValueError(name)


def act_grad(name, x):
    """d act / d x in closed form; relu is 0 at an exact 0 (what ``mp_activation_grad_f32`` gives)."""
    name = (name or "linear").replace("kgcnn>", "")
    s = torch.sigmoid(x)
    if name == "linear":
        return torch.ones_like(x)
    if name == "relu":
        return (x > 0).to(x.dtype)
    if name in ("shifted_softplus", "softplus", "softplus2"):
        return s
    if name == "swish":
        return s + x * s * (1.0 - s)
    if name == "sigmoid":
        return s * (1.0 - s)
    if name == "tanh":
        return 1.0 - torch.tanh(x) ** 2
    if name == "leaky_relu":
        return torch.where(x >= 0, torch.ones_like(x), torch.full_like(x, ALPHA))
    if name == "selu":
        return _SELU_SCALE * torch.where(x > 0, torch.ones_like(x), _SELU_ALPHA * torch.exp(torch.clamp(x, max=0.0)))
    raise ValueError(name)


def is_mean(method):
    return method in ("mean", "segment_mean", "reduce_mean")


def flat_indices(b):
    """``(recv, send)`` as global node rows (int64 tensors) of the per-graph local ``edge_indices``."""
    ns, es = np.asarray(b["node_splits"]), np.asarray(b["edge_splits"])
    idx = np.asarray(b["edge_indices"]).reshape(-1, 2) + np.repeat(ns[:-1], np.diff(es))[:, None]
    return torch.from_numpy(idx[:, 0].copy()), torch.from_numpy(idx[:, 1].copy())


def counts(recv, n, dtype):
    return torch.zeros(n, dtype=dtype).index_add_(0, recv, torch.ones(len(recv), dtype=dtype))


def pool(h, recv, n, method):
    """Rows of ``h`` added at their receiver in list order; the mean divides by the count; 0 without edges."""
    out = torch.zeros((n, h.shape[1]), dtype=h.dtype).index_add(0, recv, h)
    if is_mean(method):
        out = out / counts(recv, n, h.dtype).clamp(min=1.0)[:, None]
    return out


def bias_weight(recv, n, method, dtype):
    """``c``: what the pool makes of a constant 1 per edge."""
    c = counts(recv, n, dtype)
    return (c > 0).to(dtype) if is_mean(method) else c


# ------------------------------------------------------------------------------------------------- one edge step
def round_loop(nodes, edges, recv, send, w1, b1, w2, b2, activation, method):
    """The reference's ops, one edge at a time."""
    n = nodes.shape[0]
    out = torch.zeros((n, w2.shape[1]), dtype=nodes.dtype)
    cnt = [0] * n
    for e in range(len(recv)):
        r, s = int(recv[e]), int(send[e])
        x = torch.cat([nodes[s], nodes[r], edges[e]])          # [outgoing || ingoing || edge]
        h = x @ w1
        if b1 is not None:
            h = h + b1
        eu = act(activation, h) @ w2
        if b2 is not None:
            eu = eu + b2
        out[r] = out[r] + eu
        cnt[r] += 1
    if is_mean(method):
        out = out / torch.tensor([max(c, 1) for c in cnt], dtype=nodes.dtype)[:, None]
    return out


def mlp(x, layers):
    """``layers``: list of ``(kernel, bias or None, activation)``."""
    for kernel, bias, activation in layers:
        x = x @ kernel
        if bias is not None:
            x = x + bias
        x = act(activation, x)
    return x


def round_tensor(nodes, edges, recv, send, layers, method):
    """The reference's ops in tensor form, for an edge MLP of any depth."""
    eu = mlp(torch.cat([nodes[send], nodes[recv], edges], dim=1), layers)
    return pool(eu, recv, nodes.shape[0], method)


def split_first(nodes, edges, w1, b1):
    f, fe = nodes.shape[1], edges.shape[1]
    pj = nodes @ w1[:f]
    pi = nodes @ w1[f:2 * f]
    if b1 is not None:
        pi = pi + b1
    return pj, pi, w1[2 * f:2 * f + fe]


def edge_kernel(pj, pi, edges, wc, recv, send, activation, method, valid=None):
    """What ``mp_inorp_edge_f32`` computes: the pooled first layer, in the kernel's operation order."""
    z1 = (pj[send] + pi[recv]) + edges @ wc
    h = act(activation, z1)
    if valid is not None:
        h, recv = h[valid], recv[valid]
    return pool(h, recv, pj.shape[0], method)


def round_folded(nodes, edges, recv, send, w1, b1, w2, b2, activation, method):
    pj, pi, wc = split_first(nodes, edges, w1, b1)
    nu = edge_kernel(pj, pi, edges, wc, recv, send, activation, method) @ w2
    if b2 is not None:
        nu = nu + bias_weight(recv, nodes.shape[0], method, nodes.dtype)[:, None] * b2[None, :]
    return nu


def edge_kernel_reverse(pj, pi, edges, wc, recv, send, activation, method, g):
    """Closed forms of the reverse of ``edge_kernel``: ``(gz, Pi_bar, Pj_bar, Wc_bar, edges_bar)``."""
    n = pj.shape[0]
    z1 = (pj[send] + pi[recv]) + edges @ wc
    up = g[recv]
    if is_mean(method):
        up = up / counts(recv, n, g.dtype).clamp(min=1.0)[recv][:, None]
    gz = up * act_grad(activation, z1)
    zeros = torch.zeros((n, gz.shape[1]), dtype=g.dtype)
    return gz, zeros.index_add(0, recv, gz), zeros.index_add(0, send, gz), edges.T @ gz, gz @ wc.T


# -------------------------------------------------------------------------------------------------- edge lists
def _list(sizes, per_graph):
    ns = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    es = np.concatenate([[0], np.cumsum([len(p) for p in per_graph])]).astype(np.int64)
    idx = np.concatenate([np.asarray(p, dtype=np.int64).reshape(-1, 2) for p in per_graph], axis=0)
    return {"node_splits": ns, "edge_splits": es, "edge_indices": idx}


EDGE_LISTS = ["e0", "e1", "e31", "e32", "e33", "e65", "star70", "cut1", "batch8", "batch8_shuffled"]


def edge_list(kind):
    """A hand-made list around the 32-position tile of csrc/mp_inorp.hip.  ``eK``: one graph of 20 nodes, ``K`` edges
    sorted by receiver, node 19 never receives.  ``star70``: 5 edges into node 1, then 70 into node 3, which owns the whole
    second tile and is cut by both of its boundaries.  ``cut1``: the second receiver's 20 edges lie across position 32.
    ``batch8``: eight graphs, the third, fourth and seventh without edges; ``batch8_shuffled`` the same edges in random
    order within each graph (an unsorted list)."""
    rng = np.random.default_rng(len(kind) * 131 + sum(map(ord, kind)))
    if kind.startswith("e"):
        m = int(kind[1:])
        return _list([20], [np.stack([np.sort(rng.integers(0, 19, size=m)), rng.integers(0, 20, size=m)], axis=1)])
    if kind == "star70":
        recv = np.array([1] * 5 + [3] * 70)
        return _list([8], [np.stack([recv, rng.integers(0, 8, size=75)], axis=1)])
    if kind == "cut1":
        recv = np.array([2] * 20 + [5] * 20 + [7] * 5)
        return _list([10], [np.stack([recv, rng.integers(0, 10, size=45)], axis=1)])
    sizes, edges = [5, 7, 4, 6, 3, 8, 5, 6], [9, 14, 0, 0, 11, 20, 0, 13]
    per_graph = []
    for n, m in zip(sizes, edges):
        ij = np.stack([np.sort(rng.integers(0, n, size=m)), rng.integers(0, n, size=m)], axis=1).reshape(-1, 2)
        per_graph.append(ij[rng.permutation(m)] if kind == "batch8_shuffled" else ij)
    return _list(sizes, per_graph)


def step_operands(b, node_width, edge_width, h1, h2, seed=0, use_bias=True):
    """Node and edge features (normal times 0.5) and the edge MLP's weights for the list ``b``."""
    rng = np.random.default_rng(seed + 7 * node_width + 3 * edge_width + h1)
    n, m = int(b["node_splits"][-1]), int(b["edge_splits"][-1])
    fin = 2 * node_width + edge_width
    lim1, lim2 = np.sqrt(6.0 / (fin + h1)), np.sqrt(6.0 / (h1 + h2))
    out = {"nodes": (0.5 * rng.normal(size=(n, node_width))).astype(np.float32),
           "edges": (0.5 * rng.normal(size=(m, edge_width))).astype(np.float32),
           "w1": rng.uniform(-lim1, lim1, size=(fin, h1)).astype(np.float32),
           "w2": rng.uniform(-lim2, lim2, size=(h1, h2)).astype(np.float32), "b1": None, "b2": None}
    if use_bias:
        out["b1"] = rng.uniform(-0.1, 0.1, size=h1).astype(np.float32)
        out["b2"] = rng.uniform(-0.1, 0.1, size=h2).astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------------ the model
def _inputs(node_shape, edge_shape):
    return [{"shape": node_shape, "name": "node_attributes", "dtype": "float32", "ragged": True},
            {"shape": edge_shape, "name": "edge_attributes", "dtype": "float32", "ragged": True},
            {"shape": [None, 2], "name": "edge_indices", "dtype": "int64", "ragged": True},
            {"shape": [], "name": "graph_size", "dtype": "float32", "ragged": False}]


CONFIGS = {
    # training/hyper/hyper_esol.py: feature inputs 41 / 11, the graph state embedded, sum pooling
    "esol": {"inputs": _inputs([None, 41], [None, 11]),
             "input_embedding": {"node": {"input_dim": 95, "output_dim": 32}, "edge": {"input_dim": 15, "output_dim": 32},
                                 "graph": {"input_dim": 32, "output_dim": 32}},
             "node_mlp_args": {"units": [32, 32], "use_bias": True, "activation": ["relu", "linear"]},
             "edge_mlp_args": {"units": [32, 32], "activation": ["relu", "linear"]},
             "pooling_args": {"pooling_method": "segment_sum"}, "depth": 3, "verbose": 10,
             "output_mlp": {"use_bias": [True, True, False], "units": [32, 32, 1],
                            "activation": ["relu", "relu", "linear"]}},
    # training/hyper/hyper_mutag.py: embedded nodes and edges 16 / 8, mean pooling, a sigmoid head
    "mutag": {"inputs": _inputs([None], [None]),
              "input_embedding": {"node": {"input_dim": 60, "output_dim": 16}, "edge": {"input_dim": 4, "output_dim": 8},
                                  "graph": {"input_dim": 30, "output_dim": 16}},
              "node_mlp_args": {"units": [16, 16], "use_bias": True, "activation": ["relu", "linear"]},
              "edge_mlp_args": {"units": [16, 16], "activation": ["relu", "linear"]},
              "pooling_args": {"pooling_method": "segment_mean"}, "depth": 3, "verbose": 10,
              "output_mlp": {"use_bias": [True, True, False], "units": [16, 8, 1],
                             "activation": ["relu", "relu", "sigmoid"]}},
    # the default dictionary: a five-layer edge MLP 100 wide, which the fused route does not serve
    "default": {},
}
GRAPHS = 12
BATCH_SEED = {"esol": 61, "mutag": 62, "default": 63}
WEIGHT_SEED = {"esol": 71, "mutag": 72, "default": 73}


def model_batch(synth, name, graphs=GRAPHS):
    """Molecule graphs for configuration ``name`` with an integer graph state ``graph_number`` below 16."""
    if name == "esol":
        b = synth.cmpnn_batch(graphs, seed=BATCH_SEED[name], node_features=41, edge_features=11)
    else:
        b = synth.cmpnn_batch(graphs, seed=BATCH_SEED[name], edge_types=3)      # edge numbers 1..3 fit MUTAG's table of 4
    b["graph_number"] = np.random.default_rng(BATCH_SEED[name] + 100).integers(0, 16, size=graphs).astype(np.int64)
    return b


def spec_of(make_model_module, name, **extra):
    """What ``forward`` needs to know of a configuration: the merged keyword dictionary of the model."""
    cfg = dict(make_model_module.hyper_model_default)
    cfg.update(CONFIGS[name])
    cfg.update(extra)
    return cfg


def parity_weights(model, seed, dense_scale=0.5):
    """The weights of the parity tests for a built model: Dense kernels Glorot-uniform times ``dense_scale``, biases
    uniform in +-0.1, embeddings uniform in +-0.5.  The kernels of the output MLP behind its first ReLU are drawn
    non-negative: with signed ones the last layers cancel and the row-wise bar measures that cancellation, not the
    engine."""
    rng = np.random.default_rng(seed)
    head = model.layers[-1].name + "/"
    out = []
    for name, t in model.weights:
        shape = tuple(int(s) for s in t.shape)
        leaf = name.rsplit("/", 1)[-1]
        if leaf == "embeddings":
            v = rng.uniform(-0.5, 0.5, size=shape)
        elif leaf == "bias":
            v = rng.uniform(-0.1, 0.1, size=shape)
        else:
            limit = np.sqrt(6.0 / (shape[0] + shape[-1]))
            v = rng.uniform(-limit, limit, size=shape) * dense_scale
            if name.startswith(head) and "dense_0/" not in name:
                v = np.abs(v)
        out.append(np.asarray(v, dtype=np.float32))
    return out


def _as_list(value, n):
    return list(value) if isinstance(value, (list, tuple)) else [value] * n


def _take_mlp(ws, args):
    units = _as_list(args["units"], 1)
    acts, biases = _as_list(args.get("activation"), len(units)), _as_list(args.get("use_bias", True), len(units))
    layers = []
    for a, has_bias in zip(acts, biases):
        layers.append((ws.pop(0), ws.pop(0) if has_bias else None, a))
    return layers


def forward(weights, b, dtype, cfg, folded=True):
    """The model's output for the batch ``b``: weights in the model's order (embeddings that are used; per block the edge
    MLP, then the node MLP; the output MLP).  ``folded``: blocks with a two-layer edge MLP run ``round_folded``."""
    ws = [w if torch.is_tensor(w) else torch.tensor(np.asarray(w), dtype=dtype) for w in weights]
    recv, send = flat_indices(b)
    ns = np.asarray(b["node_splits"])
    graph_of = torch.from_numpy(np.repeat(np.arange(len(ns) - 1), np.diff(ns)))
    spec = cfg["inputs"]
    if len(spec[0]["shape"]) < 2:
        n = ws.pop(0)[torch.from_numpy(np.asarray(b["node_number"]))]
    else:
        n = torch.tensor(b["node_attributes"], dtype=dtype)
    if len(spec[1]["shape"]) < 2:
        ed = ws.pop(0)[torch.from_numpy(np.asarray(b["edge_number"]))]
    else:
        ed = torch.tensor(b["edge_attributes"], dtype=dtype)
    uenv = ws.pop(0)[torch.from_numpy(np.asarray(b["graph_number"]))]
    ev = uenv[graph_of]                                              # GatherState
    method = cfg["pooling_args"]["pooling_method"]
    for _ in range(cfg["depth"]):
        edge_layers = _take_mlp(ws, cfg["edge_mlp_args"])
        if folded and len(edge_layers) == 2 and edge_layers[1][2] in (None, "linear"):
            (w1, b1, a1), (w2, b2, _) = edge_layers
            nu = round_folded(n, ed, recv, send, w1, b1, w2, b2, a1, method)
        else:
            nu = round_tensor(n, ed, recv, send, edge_layers, method)
        n = mlp(torch.cat([n, nu, ev], dim=1), _take_mlp(ws, cfg["node_mlp_args"]))
    if cfg["output_embedding"] == "node":
        out = mlp(n, _take_mlp(ws, cfg["output_mlp"]))
    else:
        g = len(ns) - 1
        pooled = torch.zeros((g, n.shape[1]), dtype=dtype).index_add(0, graph_of, n)
        if is_mean(method):
            pooled = pooled / torch.tensor(np.maximum(np.diff(ns), 1), dtype=dtype)[:, None]
        out = mlp(pooled, _take_mlp(ws, cfg["output_mlp"]))
    assert not ws, "%d weights left over" % len(ws)
    return out


def mae(pred, target):
    return torch.abs(pred - target).mean(dim=-1).mean()


def train_target(graphs, seed=6):
    """Targets in [10, 11]: away from every output of the parity draws, so the sign in the MAE gradient is the same in
    float32 and float64."""
    return np.random.default_rng(seed).uniform(10.0, 11.0, size=(graphs, 1)).astype(np.float32)


def weight_gradients(weights, b, dtype, cfg, target):
    w = [torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for a in weights]
    loss = mae(forward(w, b, dtype, cfg), torch.tensor(target, dtype=dtype))
    grads = torch.autograd.grad(loss, w, allow_unused=True)
    return float(loss.detach()), [torch.zeros_like(t) if g is None else g for t, g in zip(w, grads)]


def sgd_steps(weights, b, cfg, target, lr, steps, dtype=torch.float64):
    """``(losses, weights after)`` of ``steps`` plain SGD steps under the MAE loss."""
    w = [np.asarray(a, dtype=np.float64) for a in weights]
    losses = []
    for _ in range(steps):
        loss, grads = weight_gradients(w, b, dtype, cfg, target)
        losses.append(loss)
        w = [a - lr * g.numpy() for a, g in zip(w, grads)]
    return losses, w
