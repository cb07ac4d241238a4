"""Torch restatement of DMPNN (kgcnn/literature/DMPNN.py:119-171) without engine imports, in the dtype of its inputs
(float32, and float64 as the budget of the parity tests): one round as a per-edge loop (``round_loop``) and in tensor form
(``round_step``), the closed forms of the round's reverse (``round_reverse``: what csrc/mp_dmpnn.hip and the
gathered-difference weight gradient compute), and the model on the weights of ``model.get_weights()`` (their order).
Indices are BATCH positions (``cmpnn_reference.flat_indices``); gradients come from torch autograd."""
import numpy as np
import torch

from cmpnn_reference import act, dense, flat_indices, seg_reduce  # noqa: F401  (flat_indices: re-exported for the tests)


def round_loop(h, h0, recv, send, rev, kernel, bias, activation="linear", edge_activation="relu", n=None):
    """One round, edge by edge: ``h'[e] = act2(act1((R[send e] - h[rev e]) W + b) + h0[e])`` with ``R[v]`` the sum of the
    states of the edges that ``v`` receives, in edge order, and no reverse term where ``rev e < 0``."""
    n = int(max(int(recv.max()), int(send.max())) + 1) if n is None else n
    received = [torch.zeros(h.shape[1], dtype=h.dtype) for _ in range(n)]
    for e in range(len(h)):
        received[int(recv[e])] = received[int(recv[e])] + h[e]
    out = []
    for e in range(len(h)):
        d = received[int(send[e])]
        if int(rev[e]) >= 0:
            d = d - h[int(rev[e])]
        z = d @ kernel
        if bias is not None:
            z = z + bias
        out.append(act(edge_activation, act(activation, z) + h0[e]))
    return torch.stack(out) if out else torch.zeros_like(h)


def difference(h, recv, send, rev, n):
    """``d[e] = R[send e] - h[rev e]``, the input of the round's Dense."""
    e_rev = torch.where((rev >= 0)[:, None], h[torch.clamp(rev, min=0)], torch.zeros_like(h))
    return seg_reduce(h, recv, n, "sum")[send] - e_rev


def round_step(h, h0, recv, send, rev, kernel, bias, activation="linear", edge_activation="relu", n=None):
    """``round_loop`` in tensor form (what the model restatement runs)."""
    n = int(max(int(recv.max()), int(send.max())) + 1) if n is None else n
    return act(edge_activation, dense(difference(h, recv, send, rev, n), kernel, bias, activation) + h0)


def round_reverse(g, y, h, recv, send, rev, kernel, n, edge_activation="relu"):
    """Closed forms of the reverse of a round with a linear Dense: ``(p, q, dW, db, h_bar)`` of the upstream gradient
    ``g`` and the round's output ``y``.  ``p`` is also the gradient of ``h0``."""
    p = g * (y > 0).to(g.dtype) if edge_activation == "relu" else g.clone()
    q = p @ kernel.T
    d = difference(h, recv, send, rev, n)
    dw, db = d.T @ p, p.sum(dim=0)
    r_bar = torch.zeros((n, h.shape[1]), dtype=g.dtype).index_add_(0, send, q)
    has = rev >= 0
    pulled = torch.zeros_like(q).index_add_(0, rev[has], q[has])      # sum over e' with rev e' = e of q[e']
    return p, q, dw, db, r_bar[recv] - pulled


def forward(weights, b, dtype, depth=5, embed_nodes=True, embed_edges=True, output_embedding="graph", method="sum",
            edge_init_activation="relu", edge_dense_activation="linear", edge_activation="relu",
            node_dense_activation="relu", mlp_use_bias=(True, True, False), mlp_activation=("relu", "relu", "linear"),
            states=False):
    """The model on ``weights`` in the model's order: the embedding tables (those of the integer inputs), the ``h0`` Dense,
    the shared edge Dense, the node Dense, the output MLP.  ``weights`` may be tensors (that require grad) or arrays."""
    ws = [w.to(dtype) if torch.is_tensor(w) else torch.as_tensor(np.asarray(w), dtype=dtype) for w in weights]
    it = iter(ws)
    recv, send, rev = flat_indices(b)
    if embed_nodes:
        n = next(it)[torch.from_numpy(np.asarray(b["node_number"], np.int64))]
    else:
        n = torch.as_tensor(np.asarray(b["node_attributes"]), dtype=dtype)
    if embed_edges:
        ed = next(it)[torch.from_numpy(np.asarray(b["edge_number"], np.int64))]
    else:
        ed = torch.as_tensor(np.asarray(b["edge_attributes"]), dtype=dtype)
    h0 = dense(torch.cat([n[send], ed], dim=1), next(it), next(it), edge_init_activation)
    w_edge, b_edge = next(it), next(it)
    h = h0
    for _ in range(depth):
        h = round_step(h, h0, recv, send, rev, w_edge, b_edge, edge_dense_activation, edge_activation, n=len(n))
    hv = dense(torch.cat([seg_reduce(h, recv, len(n), method), n], dim=1), next(it), next(it), node_dense_activation)
    out = hv
    if output_embedding == "graph":
        splits = np.asarray(b["node_splits"])
        graph = torch.from_numpy(np.repeat(np.arange(len(splits) - 1), np.diff(splits)))
        out = seg_reduce(hv, graph, len(splits) - 1, method)
    for use_bias, a in zip(mlp_use_bias, mlp_activation):
        out = dense(out, next(it), next(it) if use_bias else None, a)
    assert next(it, None) is None, "weights left over"
    return {"h": h, "node_dense": hv, "out": out} if states else out


INPUTS_FEATURES = [
    {"shape": (None, 12), "name": "node_attributes", "dtype": "float32", "ragged": True},
    {"shape": (None, 8), "name": "edge_attributes", "dtype": "float32", "ragged": True},
    {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True},
    {"shape": (None, 1), "name": "edge_indices_reverse", "dtype": "int64", "ragged": True}]

# (depth, width) of the GPU model tests: the existing model test's draw (width 32, feature inputs) and the default width
MODEL_CASES = [(3, 32), (5, 32), (3, 128), (5, 128)]
# (batch seed, weight seed) of the model-level parity cases, shared by the CPU noise-floor test and the GPU tests
MODEL_SEED = (4, 44)
NODE_SEED = (5, 45)
TRAIN_SEED = (6, 46)


TRAIN_WIDTHS = (64, 32)     # embeddings, depth 3: a served width and the existing model test's


def mse(pred, target):
    return torch.square(pred - target).mean(dim=-1).mean()


def train_target(graphs, seed=6):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=(graphs, 1)).astype(np.float32)


def weight_gradients(weights, b, dtype, loss=None, **kwargs):
    """Gradients of ``loss(out)`` (default: the sum of the outputs times fixed coefficients) for every weight; a weight
    the model does not read (an unused embedding) gets zeros."""
    w = [torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for a in weights]
    out = forward(w, b, dtype, **kwargs)
    if loss is None:
        coeff = torch.as_tensor(np.random.default_rng(17).uniform(0.5, 1.5, size=tuple(out.shape)), dtype=dtype)
        value = (out * coeff).sum()
    else:
        value = loss(out)
    grads = torch.autograd.grad(value, w, allow_unused=True)
    return [torch.zeros_like(t) if g is None else g for t, g in zip(w, grads)]


def builder_draw(synth, depth=3):
    """The draw of tests/test_gpu_models.py::test_dmpnn_builder_forward (5 SetRange graphs, 10 node and 6 edge features,
    32 units, full Glorot kernels): ``batch`` (a batch dict), ``params`` (the oracle's names), ``weights`` (the model's
    order; feature inputs have no embedding tables), ``kwargs`` (``make_model``'s)."""
    b = synth.qm9_like_batch(num_graphs=5, seed=23)
    rng = np.random.default_rng(24)
    n, m = int(b["node_splits"][-1]), int(b["edge_splits"][-1])
    fn, fe, units = 10, 6, 32
    x = rng.normal(size=(n, fn)).astype(np.float32)
    e = rng.normal(size=(m, fe)).astype(np.float32)
    pairs = np.full((m, 1), -1, dtype=np.int64)
    es = b["edge_splits"]
    for g in range(5):
        seg = b["edge_indices"][es[g]:es[g + 1]]
        pos = {(int(i), int(j)): k for k, (i, j) in enumerate(seg)}
        for k, (i, j) in enumerate(seg):
            pairs[es[g] + k, 0] = pos.get((int(j), int(i)), -1)
    p, arrays = {}, []

    def add(key, fin, fout):
        p[key + "/kernel"] = synth.glorot_uniform(rng, fin, fout)
        p[key + "/bias"] = (rng.normal(size=fout) * 0.1).astype(np.float32)
        arrays.extend([p[key + "/kernel"], p[key + "/bias"]])
    add("h0", fn + fe, units); add("edge", units, units); add("node", units + fn, units)
    for k, (fin, fout, has_bias) in enumerate(((units, 16, True), (16, 8, True), (8, 1, False))):
        p["output_mlp/%d/kernel" % k] = synth.glorot_uniform(rng, fin, fout)
        arrays.append(p["output_mlp/%d/kernel" % k])
        if has_bias:
            p["output_mlp/%d/bias" % k] = (rng.normal(size=fout) * 0.1).astype(np.float32)
            arrays.append(p["output_mlp/%d/bias" % k])
    batch = {"node_attributes": x, "edge_attributes": e, "edge_indices": b["edge_indices"], "edge_indices_reverse": pairs,
             "node_splits": b["node_splits"], "edge_splits": es}
    spec = [dict(s) for s in INPUTS_FEATURES]
    spec[0]["shape"], spec[1]["shape"] = (None, fn), (None, fe)
    kwargs = dict(inputs=spec, edge_initialize={"units": units}, edge_dense={"units": units}, node_dense={"units": units},
                  depth=depth, output_mlp={"units": [16, 8, 1]}, verbose=30)
    return {"batch": batch, "params": p, "weights": arrays, "kwargs": kwargs}


def model_case(synth, make_model, depth, width):
    """``(model, batch, weights, forward keywords)`` of a MODEL_CASES entry: width 32 is the existing model test's draw
    (feature inputs, full Glorot kernels), any other width 12 molecule graphs with embeddings under ``parity_weights``."""
    if width == 32:
        case = builder_draw(synth, depth)
        return make_model(**case["kwargs"]), case["batch"], case["weights"], dict(depth=depth, embed_nodes=False,
                                                                                 embed_edges=False)
    model = make_model(**model_kwargs(width, depth))
    return model, synth.cmpnn_batch(12, seed=MODEL_SEED[0]), parity_weights(model, MODEL_SEED[1]), dict(depth=depth)


def model_kwargs(width, depth=5, features=False, **extra):
    unit = lambda activation: {"units": width, "use_bias": True, "activation": activation}
    kw = dict(edge_initialize=unit("relu"), edge_dense=unit("linear"), node_dense=unit("relu"), depth=depth, verbose=30)
    if features:
        kw["inputs"] = [dict(spec) for spec in INPUTS_FEATURES]
    kw.update(extra)
    return kw


def parity_weights(model, seed=41, dense_scale=0.5):
    """The weights of the parity tests for a built model (anything with ``.weights`` as (name, tensor) pairs): Dense kernels
    Glorot-uniform times ``dense_scale`` (the shared edge kernel is applied ``depth`` times to a sum over neighbours: with
    O(1) weights the states grow per round and two float32 pipelines part), biases uniform in +-0.1,
    embeddings uniform in +-0.5."""
    rng = np.random.default_rng(seed)
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
        out.append(np.asarray(v, dtype=np.float32))
    return out


def round_case(edges, width, reverse="mix", seed=0, shuffle=False):
    """Two graphs (one for fewer than two edges) that share ``edges`` directed edges over 70 + 45 nodes, receiver-sorted
    lists (``shuffle``: in random order) with random senders; node 69 of the first graph sends nothing.  Reverse positions
    are drawn over the whole graph's list (they point into other tiles and need not be an involution): ``mix`` - a third
    without a reverse (-1), ``none`` - all -1, ``self`` - every edge its own reverse, ``twice`` - as ``mix``, and the first
    two edges of every graph name the same reverse.  States are normal times 0.5."""
    rng = np.random.default_rng(seed + 7 * edges + width)
    sizes = [70, 45] if edges >= 2 else [70]
    counts = [edges - edges // 3, edges // 3] if edges >= 2 else [edges]
    idx, pair = [], []
    for gi, (n, m) in enumerate(zip(sizes, counts)):
        send = rng.integers(0, n - 1 if gi == 0 else n, size=m)
        ij = np.stack([np.sort(rng.integers(0, n, size=m)), send], axis=1)
        if shuffle:
            ij = ij[rng.permutation(m)]
        idx.append(ij)
        if reverse == "none":
            pr = np.full(m, -1)
        elif reverse == "self":
            pr = np.arange(m)
        else:
            pr = np.where(rng.random(m) < 1 / 3, -1, rng.integers(0, max(m, 1), size=m))
            if reverse == "twice" and m >= 2:
                pr[0] = pr[1] = m - 1
        pair.append(pr)
    ns, es = np.concatenate([[0], np.cumsum(sizes)]), np.concatenate([[0], np.cumsum(counts)])
    b = {"edge_indices": np.concatenate(idx).astype(np.int64).reshape(-1, 2),
         "edge_indices_reverse": np.concatenate(pair).astype(np.int64).reshape(-1, 1), "node_splits": ns, "edge_splits": es}
    b["h"] = (0.5 * rng.normal(size=(edges, width))).astype(np.float32)
    b["h0"] = (0.5 * rng.normal(size=(edges, width))).astype(np.float32)
    return b
