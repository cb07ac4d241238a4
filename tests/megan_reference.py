"""Differentiable torch-CPU restatement of MEGAN (kgcnn/literature/MEGAN.py:251-327, its ``train_step`` :359-451, and
``regression_augmentation`` :329-357), in float64 or float32: the budget and the float32 twin of the GPU tests.  TEST
INFRASTRUCTURE: no engine imports.

Written from the reference's op sequence: the attention layers are ``gat_reference.multi_head`` (MultiHeadGATV2Layer with
its final activation), their ``(M, K, 1)`` logits are concatenated on the last axis and summed over it, the sigmoid of the
sum is the edge importance; two mean pools of it (one per index column) are averaged, multiplied with the sigmoid of the
node-importance Dense chain, and the embeddings are pooled per graph once per channel, weighted by that channel.

Parameters are dictionaries in ``model.weights`` order: ``embed_n`` (if any), ``att{i}/head{k}/...`` with the keys of
``gat_reference.head_params``, ``imp/{j}/kernel|bias``, ``final/{j}/kernel|bias``.  ``idx`` is the flat ``(M, 2)`` int64
list of the whole batch.  TensorFlow is not available to the suite, so there is no recorded output of the reference: this
restatement is the yardstick, as ``gat_reference`` is for GAT.
"""
import numpy as np
import torch

from gat_reference import ACTIVATIONS, dense, glorot, head_params, multi_head, params_to, sub  # noqa: F401

EPS = 1e-7   # tf.keras.backend.epsilon()


def _t(a, dtype):
    return a.to(dtype) if torch.is_tensor(a) else torch.tensor(np.asarray(a), dtype=dtype)


# ----------------------------------------------------------------------------------------------- the tail, op by op
def edge_importance(logits):
    """``sigmoid(sum_l logits_l)`` over a list of ``(M, K)`` tensors, summed in layer order."""
    total = logits[0]
    for a in logits[1:]:
        total = total + a
    return torch.sigmoid(total)


def segment_mean(data, seg, rows):
    """``PoolingLocalEdges(pooling_method='mean')``: a segment without rows gives 0."""
    s = torch.zeros((rows,) + tuple(data.shape[1:]), dtype=data.dtype).index_add(0, seg, data)
    cnt = torch.zeros(rows, dtype=data.dtype).index_add(0, seg, torch.ones(len(seg), dtype=data.dtype))
    return s / torch.clamp(cnt, min=1.0)[:, None]


def graph_pool(values, node_splits, method):
    """``PoolingNodes``: all ``G`` rows (an empty graph gives 0); the caller trims trailing empty graphs."""
    s = np.asarray(node_splits, np.int64)
    g = len(s) - 1
    if method == "max":
        rows = [values[s[b]:s[b + 1]].max(dim=0).values if s[b + 1] > s[b] else torch.zeros(values.shape[1], dtype=values.dtype)
                for b in range(g)]
        return torch.stack(rows) if rows else torch.zeros((0, values.shape[1]), dtype=values.dtype)
    graph = torch.from_numpy(np.repeat(np.arange(g), s[1:] - s[:-1]))
    pooled = torch.zeros((g, values.shape[1]), dtype=values.dtype).index_add(0, graph, values)
    if method == "mean":
        pooled = pooled / torch.clamp(torch.from_numpy((s[1:] - s[:-1]).astype(np.float64)).to(values.dtype), min=1.0)[:, None]
    return pooled


def trimmed_rows(node_splits):
    s = np.asarray(node_splits, np.int64)
    rows = len(s) - 1
    while rows > 0 and s[rows] == s[rows - 1]:
        rows -= 1
    return rows


def readout(x, z, ei, idx, node_splits, pooling="sum"):
    """The tail behind the edge importances: ``(p (N, K), ni (N, K), out (G, K W))``."""
    idx = torch.as_tensor(np.asarray(idx), dtype=torch.int64).reshape(-1, 2)
    n, k = x.shape[0], z.shape[1]
    pooled_in = segment_mean(ei, idx[:, 0], n)
    pooled_out = segment_mean(ei, idx[:, 1], n)
    p = (pooled_out + pooled_in) / 2
    ni = torch.sigmoid(z) * p
    outs = [graph_pool(x * ni[:, c:c + 1], node_splits, pooling) for c in range(k)]
    return p, ni, torch.cat(outs, dim=-1)


# ----------------------------------------------------------------------------------------------- the model
def config(units, k=2, concat=True, use_edge_features=True, importance_units=(), final_units=(1,),
           final_activation="linear", final_pooling="sum", activation="kgcnn>leaky_relu", use_bias=True,
           regression_limits=None, regression_reference=None, importance_factor=0.0, importance_multiplier=10.0,
           sparsity_factor=0.0, embed=None):
    """The restatement's view of the constructor arguments.  ``embed``: ``(rows, width)`` of a node embedding table."""
    return dict(units=list(units), k=k, concat=concat, use_edge_features=use_edge_features,
                importance_units=list(importance_units), final_units=list(final_units), final_activation=final_activation,
                final_pooling=final_pooling, activation=activation, use_bias=use_bias, regression_limits=regression_limits,
                regression_reference=regression_reference, importance_factor=importance_factor,
                importance_multiplier=importance_multiplier, sparsity_factor=sparsity_factor, embed=embed)


def model_kwargs(cfg):
    """Keyword arguments of ``gcnn_keras_amd.literature.MEGAN.MEGAN`` for a configuration."""
    kw = dict(units=cfg["units"], importance_channels=cfg["k"], concat_heads=cfg["concat"],
              use_edge_features=cfg["use_edge_features"], importance_units=cfg["importance_units"],
              final_units=cfg["final_units"], final_activation=cfg["final_activation"], final_pooling=cfg["final_pooling"],
              activation=cfg["activation"], use_bias=cfg["use_bias"], regression_limits=cfg["regression_limits"],
              regression_reference=cfg["regression_reference"], importance_factor=cfg["importance_factor"],
              importance_multiplier=cfg["importance_multiplier"], sparsity_factor=cfg["sparsity_factor"])
    if cfg["embed"] is not None:
        kw["input_embedding"] = {"node": {"input_dim": cfg["embed"][0], "output_dim": cfg["embed"][1],
                                          "use_embedding": True}}
    return kw


def model_params(rng, cfg, fn, fe):
    """Glorot kernels at scale 1 and biases in +-0.1 in ``model.weights`` order; ``fn`` / ``fe``: node and edge feature
    widths (``fn`` is ignored with an embedding)."""
    small = lambda size: rng.uniform(-0.1, 0.1, size=size).astype(np.float32)
    p = {}
    if cfg["embed"] is not None:
        p["embed_n"] = rng.uniform(-0.5, 0.5, size=cfg["embed"]).astype(np.float32)
        fn = cfg["embed"][1]
    width, k, bias = fn, cfg["k"], cfg["use_bias"]
    d = fe if cfg["use_edge_features"] else 0
    for i, u in enumerate(cfg["units"]):
        for h in range(k):
            for name, v in head_params(rng, width, u, d, True, bias).items():
                p["att%d/head%d/%s" % (i, h, name)] = v
        width = u * k if cfg["concat"] else u
    fan = width
    for j, u in enumerate(cfg["importance_units"] + [k]):
        p["imp/%d/kernel" % j] = glorot(rng, fan, u)
        if bias:
            p["imp/%d/bias" % j] = small(u)
        fan = u
    fan = width * k
    for j, u in enumerate(cfg["final_units"]):
        p["final/%d/kernel" % j] = glorot(rng, fan, u)
        if bias:
            p["final/%d/bias" % j] = small(u)
        fan = u
    return p


def model_forward(params, cfg, node_attr, edge_attr, idx, node_splits):
    """``MEGAN.call`` with ``return_importances=True``: ``(out (G', F), ni (N, K), ei (M, K))``, ``G'`` without trailing
    empty graphs.  Integer ``node_attr`` indexes ``params['embed_n']``."""
    if not torch.is_floating_point(node_attr):
        node_attr = params["embed_n"][node_attr.reshape(-1)]
    k, act = cfg["k"], cfg["activation"]
    x, alphas = node_attr, []
    for i in range(len(cfg["units"])):
        heads = [sub(params, "att%d/head%d/" % (i, h)) for h in range(k)]
        x, alpha = multi_head(x, edge_attr, idx, heads, act=act, concat=cfg["concat"],
                              use_edge_features=cfg["use_edge_features"], use_final_activation=True)
        alphas.append(alpha)                                   # (M, K, 1)
    ei = torch.sigmoid(torch.cat(alphas, dim=-1).sum(dim=-1))  # concatenated on the last axis and summed over it
    z = x
    acts = ["relu"] * len(cfg["importance_units"]) + ["linear"]
    for j, a in enumerate(acts):
        z = dense(z, params["imp/%d/kernel" % j], params.get("imp/%d/bias" % j), a)
    _, ni, out = readout(x, z, ei, idx, node_splits, cfg["final_pooling"])
    out = out[:trimmed_rows(node_splits)]
    acts = ["relu"] * len(cfg["final_units"])
    acts[-1] = cfg["final_activation"]
    for j, a in enumerate(acts):
        out = dense(out, params["final/%d/kernel" % j], params.get("final/%d/bias" % j), a)
    if cfg["regression_limits"] is not None:
        out = out + cfg["regression_reference"]
    return out, ni, ei


# ----------------------------------------------------------------------------------------------- the training loss
def shifted_sigmoid(x, shift=5.0, multiplier=1.0):
    return torch.sigmoid((x - shift) / multiplier)


def regression_augmentation(y, cfg):
    """``(samples, mask)`` of kgcnn/literature/MEGAN.py:329-357 for ``y`` (B, 1)."""
    ref = cfg["regression_reference"]
    width = abs(cfg["regression_limits"][1] - cfg["regression_limits"][0])
    dist = (y - ref).abs() * cfg["importance_multiplier"] / (0.5 * width)
    lo = torch.where(y < ref, 1.0, 0.0).to(y.dtype)
    hi = torch.where(y > ref, 1.0, 0.0).to(y.dtype)
    return torch.cat([dist, dist], dim=-1), torch.cat([lo, hi], dim=-1)


def keras_loss(name, pred, y):
    """tf.keras losses with reduction sum-over-batch-size: the mean over the last axis, then over the samples."""
    if name == "mean_squared_error":
        return torch.square(pred - y).mean(dim=-1).mean()
    if name == "mean_absolute_error":
        return (pred - y).abs().mean(dim=-1).mean()
    if name == "binary_crossentropy":
        p = pred.clamp(EPS, 1 - EPS)
        return -(y * torch.log(p + EPS) + (1 - y) * torch.log(1 - p + EPS)).mean(dim=-1).mean()
    raise KeyError(name)


def total_loss(out, ni, y, node_splits, cfg, loss="mean_squared_error"):
    """``(total, exp_loss)`` of the train step: compiled loss + ``sparsity_factor * mean |ni|`` + ``importance_factor *``
    the explanation loss (``exp_loss`` is that last term, 0 without it)."""
    total = keras_loss(loss, out, y) + cfg["sparsity_factor"] * ni.abs().mean()
    exp = torch.zeros((), dtype=out.dtype)
    if cfg["importance_factor"] != 0:
        outs = graph_pool(ni, node_splits, cfg["final_pooling"])[:trimmed_rows(node_splits)]
        if cfg["regression_limits"] is not None:
            samples, mask = regression_augmentation(y, cfg)
            exp = cfg["k"] * keras_loss("mean_absolute_error", outs * mask, samples * mask)
        else:
            exp = keras_loss("binary_crossentropy", shifted_sigmoid(outs, cfg["importance_multiplier"], 1.0), y)
        exp = exp * cfg["importance_factor"]
        total = total + exp
    return total, exp


# ----------------------------------------------------------------------------------------------- model cases
FN, FE = 12, 6


def model_cases():
    """name -> configuration of every model parity case of tests/test_gpu_megan.py.  ``u5-3-k2`` is the reference's own
    test size; its embeddings are 6 wide (3 units x 2 heads), which the fused readout does not serve (a multiple of 4),
    so ``u5-4-k2`` stands beside it for 'attention on the layer sequence, readout fused'."""
    return {
        "u32x3-k2-concat": config([32, 32, 32], k=2, concat=True),
        "u64-32-k4-avg-embed-noedge": config([64, 32], k=4, concat=False, use_edge_features=False, importance_units=[16],
                                             final_units=[8, 3], final_pooling="mean", embed=(95, 16)),
        "u5-3-k2": config([5, 3], k=2, concat=True),
        "u5-4-k2": config([5, 4], k=2, concat=True, final_units=[3], regression_limits=(-1.0, 1.0), regression_reference=0.5),
        "u32-k8-embed": config([32], k=8, concat=True, final_pooling="mean", embed=(95, 16)),
    }


def unserved_cases():
    """Configurations outside the fused readout: they take the layer sequence."""
    return {"max-pool": config([32, 32], k=2, final_pooling="max"), "k9": config([32], k=9)}


def model_case(cfg, seed=21, num_graphs=6):
    """``(batch, parameters)``: 6 QM9-like graphs with N(0, 1) features (``synth.megan_batch``; the numbers of
    ``node_type`` with an embedding), ``flat`` = the batch-wide index list."""
    from gcnn_keras_amd import synth
    b = synth.megan_batch(num_graphs=num_graphs, seed=seed, node_features=FN, edge_features=FE)
    b["flat"] = b["edge_indices"] + np.repeat(b["node_splits"][:-1], np.diff(b["edge_splits"]))[:, None]
    b["x"] = b["node_type"] if cfg["embed"] is not None else b["node_attributes"]
    b["e"] = b["edge_attributes"]
    return b, model_params(np.random.default_rng(seed + 1), cfg, FN, FE)


def model_restate(params, cfg, b, dtype, requires_grad=False):
    """``(out, ni, ei)`` torch tensors of a case in ``dtype`` (and the parameter leaves when ``requires_grad``)."""
    p = params_to(params, dtype, requires_grad)
    x = torch.from_numpy(b["x"].astype(np.int64)) if cfg["embed"] is not None else _t(b["x"], dtype)
    res = model_forward(p, cfg, x, _t(b["e"], dtype), b["flat"], b["node_splits"])
    return (res, p) if requires_grad else res


# ----------------------------------------------------------------------------------------------- kernel cases
NODE_TILE = 64   # MP_MEGAN_NODE_TILE of include/mpengine/megan.h


def directed_edges():
    """Six nodes, ``[receiver, sender]``: node 0 only sends (out-degree 3), node 5 only receives (in-degree 3), node 4 is
    isolated; in-degrees (0, 3, 2, 2, 0, 3) against out-degrees (3, 2, 3, 2, 0, 0)."""
    return np.array([[1, 0], [2, 0], [3, 0], [5, 1], [5, 2], [5, 3], [2, 1], [3, 2], [1, 3], [1, 2]], np.int64)


def kernel_graphs(kind, order, seed):
    import topologies as topo
    if kind == "hub":          # degree 1000 as a receiver, self loops and duplicate edges, empty graphs around
        return topo.with_empty_graphs([(1100, topo.hub_edges(1100, topo.STANDARD_DEGREES, seed, True, True, order)),
                                       (1, np.zeros((0, 2), np.int64)),
                                       (60, topo.hub_edges(60, (2, 96, 5), seed + 1, True, True, order))])
    if kind == "hubsend":      # the same lists with the columns exchanged: degree 1000 as a sender
        return [(n, topo.swap_columns(e)) for n, e in kernel_graphs("hub", order, seed)]
    if kind == "tiles":        # one below, at and one above the node tile; a lone node; empty graphs
        sizes = (NODE_TILE - 1, NODE_TILE, NODE_TILE + 1, 2 * NODE_TILE + 3)
        graphs = [(n, topo.two_neighbour_edges(n)) for n in sizes] + [(1, np.zeros((0, 2), np.int64))]
        if order == "shuffled":
            rng = np.random.default_rng(seed)
            graphs = [(n, e[rng.permutation(len(e))]) for n, e in graphs]
        return topo.with_empty_graphs(graphs)
    if kind == "directed":
        e = directed_edges()
        if order == "shuffled":
            e = e[np.random.default_rng(seed).permutation(len(e))]
        return [(0, np.zeros((0, 2), np.int64)), (6, e), (6, e[::-1].copy())]
    raise KeyError(kind)


def kernel_cases():
    """name -> keyword arguments of ``kernel_case``: K 1 / 2 / 8, W 4 / 32 / 36 / 64 / 512, L 1 / 3 / 8, sum and mean."""
    return {
        "hub-sorted-k2-w64-l3-sum": dict(kind="hub", order="sorted", k=2, w=64, layers=3, pooling="sum"),
        "hub-shuffled-k8-w36-l8-mean": dict(kind="hub", order="shuffled", k=8, w=36, layers=8, pooling="mean"),
        "hub-shuffled-k2-w512-l1-sum": dict(kind="hub", order="shuffled", k=2, w=512, layers=1, pooling="sum"),
        "hubsend-shuffled-k1-w4-l1-mean": dict(kind="hubsend", order="shuffled", k=1, w=4, layers=1, pooling="mean"),
        "hubsend-sorted-k8-w32-l3-sum": dict(kind="hubsend", order="sorted", k=8, w=32, layers=3, pooling="sum"),
        "tiles-sorted-k2-w32-l1-mean": dict(kind="tiles", order="sorted", k=2, w=32, layers=1, pooling="mean"),
        "tiles-shuffled-k8-w512-l3-sum": dict(kind="tiles", order="shuffled", k=8, w=512, layers=3, pooling="sum"),
        "directed-sorted-k1-w36-l8-sum": dict(kind="directed", order="sorted", k=1, w=36, layers=8, pooling="sum"),
        "directed-shuffled-k2-w4-l3-mean": dict(kind="directed", order="shuffled", k=2, w=4, layers=3, pooling="mean"),
    }


def kernel_case(kind="hub", order="sorted", k=2, w=64, layers=3, pooling="sum", seed=0):
    """Inputs of the four kernels: ``logits`` (``layers`` x (M, K), summing to N(0, 1)), ``z`` (N, K), ``x`` (N, W) and the
    upstream gradients ``g_out`` (G, K W), ``g_ni`` (N, K), ``g_ei`` (M, K)."""
    import topologies as topo
    b = topo.batch(kernel_graphs(kind, order, seed))
    rng = np.random.default_rng(5000 + seed + 11 * k + w)
    n, m, g = int(b["row_splits"][-1]), len(b["flat"]), len(b["row_splits"]) - 1
    f32 = lambda a: a.astype(np.float32)
    b.update(logits=[f32(rng.normal(size=(m, k)) / np.sqrt(layers)) for _ in range(layers)],
             z=f32(rng.normal(size=(n, k))), x=f32(rng.normal(size=(n, w))), g_out=f32(rng.normal(size=(g, k * w))),
             g_ni=f32(rng.normal(size=(n, k))), g_ei=f32(rng.normal(size=(m, k))), k=k, w=w, pooling=pooling, rows=n)
    return b


def kernel_restate(case, dtype, with_g_ni=True, with_g_ei=True):
    """numpy ``dict(ei, p, ni, out, x_bar, z_bar, s_bar)``: the forward, and autograd's reverse for the case's upstream
    gradients (``g_ni`` / ``g_ei`` absent when switched off).  ``s_bar`` is the gradient of every logit tensor."""
    logits = [_t(a, dtype).requires_grad_(True) for a in case["logits"]]
    z, x = _t(case["z"], dtype).requires_grad_(True), _t(case["x"], dtype).requires_grad_(True)
    ei = edge_importance(logits)
    p, ni, out = readout(x, z, ei, case["flat"], case["row_splits"], case["pooling"])
    res = {"ei": ei, "p": p, "ni": ni, "out": out}
    scalar = (out * _t(case["g_out"], dtype)).sum()
    if with_g_ni:
        scalar = scalar + (ni * _t(case["g_ni"], dtype)).sum()
    if with_g_ei:
        scalar = scalar + (ei * _t(case["g_ei"], dtype)).sum()
    grads = torch.autograd.grad(scalar, [x, z] + logits, allow_unused=True)
    zero = lambda g, like: torch.zeros_like(like) if g is None else g
    res.update(x_bar=zero(grads[0], x), z_bar=zero(grads[1], z), s_bar=zero(grads[2], logits[0]))
    for g in grads[3:]:
        assert torch.equal(zero(g, logits[0]), res["s_bar"])     # one gradient for every layer's logits
    return {name: v.detach().numpy() for name, v in res.items()}
