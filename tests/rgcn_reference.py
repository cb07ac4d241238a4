"""Torch-CPU restatement of RGCN and GNNFilm in the reference's op order (kgcnn/literature/RGCN.py:96-103,
kgcnn/literature/GNNFilm.py:93-102, kgcnn/layers/relational.py:204-238), runnable in float32 and float64: per edge the
``batch_dot`` of the gathered features with the gathered kernel, then multiply, pool, add, activation.  A relation outside
``[0, num_relations)`` gathers a zero kernel (TF's GPU gather).  Also the kernel cases of tests/test_gpu_rgcn.py (index
lists from tests/topologies.py) and the weights its model tests use.  No engine import."""
import numpy as np
import torch

import topologies as topo


# ------------------------------------------------------------------------------------------------------------- ops
def activation(name, x):
    if name in (None, "linear"):
        return x
    if name == "relu":
        return torch.relu(x)
    if name == "swish":
        return x * torch.sigmoid(x)
    if name == "sigmoid":
        return torch.sigmoid(x)
    if name == "tanh":
        return torch.tanh(x)
    if name == "softplus":
        return torch.nn.functional.softplus(x)
    if name == "softmax":
        return torch.softmax(x, dim=-1)
    raise KeyError(name)


def effective_kernel(kernel, lin_bases=None, num_blocks=None):
    """relational.py:204-217: block-diagonal expansion, then ``tensordot(lin_bases, kernel, [1, 0])``."""
    if num_blocks is not None:
        kernel = torch.stack([torch.block_diag(*[kernel[b, i] for i in range(kernel.shape[1])])
                              for b in range(kernel.shape[0])])
    if lin_bases is not None:
        kernel = torch.tensordot(lin_bases, kernel, dims=([1], [0]))
    return kernel


def relational_dense(x, rel, kernel, bias=None, act="linear", lin_bases=None, num_blocks=None):
    """relational.py:231-238: ``act(batch_dot(x, gather(kernel, rel)) + bias)``; out-of-range relations: zero kernel."""
    w = effective_kernel(kernel, lin_bases, num_blocks)
    nrel = w.shape[0]
    padded = torch.cat([w, torch.zeros_like(w[:1])], dim=0)
    rel = torch.as_tensor(rel, dtype=torch.int64)
    safe = torch.where((rel >= 0) & (rel < nrel), rel, torch.full_like(rel, nrel))
    y = torch.einsum("ek,eku->eu", x, padded[safe])
    if bias is not None:
        y = y + bias
    return activation(act, y)


def pool_sum(messages, recv, n):
    return torch.zeros((n, messages.shape[1]), dtype=messages.dtype).index_add(0, torch.as_tensor(recv), messages)


def rgcn_block(n, flat, weights, rel, p, act0="linear", act="swish", num_blocks=None):
    """RGCN.py:97-103.  ``p``: ``w0, b0`` (Dense), ``kernel, lin_bases, bias`` (RelationalDense); None where absent."""
    recv, send = torch.as_tensor(flat[:, 0]), torch.as_tensor(flat[:, 1])
    n_j = n[send]
    h0 = n @ p["w0"]
    if p.get("b0") is not None:
        h0 = h0 + p["b0"]
    h0 = activation(act0, h0)
    h_j = relational_dense(n_j, rel, p["kernel"], p.get("bias"), "linear", p.get("lin_bases"), num_blocks)
    m = h_j * weights if weights is not None else h_j
    h = pool_sum(m, recv, n.shape[0])
    return activation(act, h + h0)


def film_block(n, flat, rel, p, act_m="sigmoid", act="swish", num_blocks=None):
    """GNNFilm.py:94-102.  ``p``: ``wg, bg, wt, bt`` (gamma, beta), ``kernel, lin_bases, bias`` (message)."""
    recv, send = torch.as_tensor(flat[:, 0]), torch.as_tensor(flat[:, 1])
    n_i, n_j = n[recv], n[send]
    gamma = relational_dense(n_i, rel, p["wg"], p.get("bg"), act_m)
    beta = relational_dense(n_i, rel, p["wt"], p.get("bt"), act_m)
    h_j = relational_dense(n_j, rel, p["kernel"], p.get("bias"), "linear", p.get("lin_bases"), num_blocks)
    m = h_j * gamma
    m = m + beta
    h = pool_sum(m, recv, n.shape[0])
    return activation(act, h)


# ------------------------------------------------------------------------------------------------------------ models
def model_forward(kind, weights, b, dtype, depth, embed=True, num_bases=None, num_blocks=None, output_embedding="graph",
                  mlp_activations=("swish", "linear"), act_m="sigmoid", act="swish", blocks_out=None):
    """The whole model on the weights in ``model.weights`` order (every ``use_bias`` on).  ``b``: ``x`` (numbers or
    features), ``flat`` (E, 2) batch-shifted, ``edge_weights`` (E, 1), ``edge_relations`` (E), ``node_splits``.
    ``blocks_out`` (a list) collects the node states after every block."""
    it = iter(weights)

    def nxt():
        w = next(it)
        return w.to(dtype) if torch.is_tensor(w) else torch.tensor(np.asarray(w), dtype=dtype)

    if embed:
        n = nxt()[torch.as_tensor(np.asarray(b["x"]).astype(np.int64))]
    else:
        n = torch.as_tensor(b["x"]).to(dtype)
    ew = torch.as_tensor(b["edge_weights"]).to(dtype) if kind == "rgcn" else None
    for _ in range(depth):
        p = {}
        if kind == "rgcn":
            p["w0"], p["b0"] = nxt(), nxt()
        else:
            p["wg"], p["bg"], p["wt"], p["bt"] = nxt(), nxt(), nxt(), nxt()
        p["kernel"] = nxt()
        p["lin_bases"] = nxt() if num_bases is not None else None
        p["bias"] = nxt()
        if kind == "rgcn":
            n = rgcn_block(n, b["flat"], ew, b["edge_relations"], p, "linear", act, num_blocks)
        else:
            n = film_block(n, b["flat"], b["edge_relations"], p, act_m, act, num_blocks)
        if blocks_out is not None:
            blocks_out.append(n)
    if output_embedding == "graph":
        ns = np.asarray(b["node_splits"])
        rows = [n[ns[g]:ns[g + 1]].mean(dim=0) if ns[g + 1] > ns[g] else torch.zeros(n.shape[1], dtype=dtype)
                for g in range(len(ns) - 1)]
        n = torch.stack(rows)
    for name in mlp_activations:
        n = activation(name, n @ nxt() + nxt())
    assert next(it, None) is None, "weights left over"
    return n


def parity_weights(model, seed):
    """Weights for a built model, as a list in ``model.weights`` order: kernels Glorot-uniform on their last two axes,
    ``lin_bases`` uniform in +-1 / sqrt(num_bases), biases in +-0.1, embeddings in +-0.5."""
    rng = np.random.default_rng(seed)
    out = []
    for name, t in model.weights:
        shape = tuple(int(s) for s in t.shape)
        leaf = name.rsplit("/", 1)[-1]
        if leaf == "embeddings":
            v = rng.uniform(-0.5, 0.5, size=shape)
        elif leaf == "bias":
            v = rng.uniform(-0.1, 0.1, size=shape)
        elif leaf == "lin_bases":
            v = rng.uniform(-1.0, 1.0, size=shape) / np.sqrt(shape[1])
        else:
            lim = np.sqrt(6.0 / (shape[-2] + shape[-1]))
            v = rng.uniform(-lim, lim, size=shape)
        out.append(np.asarray(v, dtype=np.float32))
    return out


# ------------------------------------------------------------------------------------------------------ kernel cases
def _graphs(kind, order, seed):
    hub = lambda n: (n, topo.hub_edges(n, topo.SMALL_DEGREES, seed, True, True, order))
    if kind in ("n15", "n16", "n17"):       # the six hub receivers (degrees 1 .. 100) sit in ONE 16-receiver tile
        return [hub(int(kind[1:]))]
    if kind == "n33":                       # two full tiles and one row; empty graphs first, in the middle and last
        return topo.with_empty_graphs([hub(17), (16, topo.two_neighbour_edges(16))])
    if kind == "n1":
        return [(1, np.zeros((3, 2), np.int64))]            # three self loops
    if kind == "n1-e0":
        return [(1, np.zeros((0, 2), np.int64))]
    if kind == "n17-e0":
        return [(17, np.zeros((0, 2), np.int64))]
    if kind == "chunks":                    # 560 positions in one tile: the 256-position chunks cut receivers 2 and 4
        e = topo.degree_edges(20, (100, 0, 157, 3, 300), seed)
        if order == "shuffled":
            e = e[np.random.default_rng(seed).permutation(len(e))]
        return [(20, e)]
    raise KeyError(kind)


def kernel_cases():
    """name -> keyword arguments of ``kernel_case``."""
    return {
        "n17-sorted-r20": dict(kind="n17", r=20, relations="unused5", ku=(64, 64)),
        "n17-shuffled-r3-oor": dict(kind="n17", order="shuffled", r=3, oor=True, ku=(32, 128), act0="relu"),
        "n15-sorted-r1": dict(kind="n15", r=1, ku=(128, 32), bias=False, weights=False),
        "n16-shuffled-r64": dict(kind="n16", order="shuffled", r=64, relations="distinct", ku=(64, 64), bias=False),
        "n33-shuffled-r64-empty-graphs": dict(kind="n33", order="shuffled", r=64, relations="distinct", oor=True,
                                              ku=(64, 64), act_m="tanh"),
        "n33-sorted-r20-one-relation": dict(kind="n33", r=20, relations="one", ku=(32, 128), weights=False),
        "n17-sorted-r20-oor-nobias": dict(kind="n17", r=20, oor=True, ku=(128, 32), bias=False, act="tanh"),
        "n1-self-loops-r3": dict(kind="n1", r=3, ku=(64, 64)),
        "n1-e0": dict(kind="n1-e0", r=3, ku=(32, 128)),
        "n17-e0": dict(kind="n17-e0", r=20, ku=(64, 64)),
        "chunks-sorted-r20-oor": dict(kind="chunks", r=20, oor=True, ku=(64, 64)),
        "chunks-shuffled-r64": dict(kind="chunks", order="shuffled", r=64, ku=(128, 32), bias=False),
    }


def kernel_case(kind, r, ku, order="sorted", relations="random", oor=False, bias=True, weights=True, act0="linear",
                act_m="sigmoid", act="swish", seed=5):
    """Inputs and weights of one block for both modes.  ``relations``: "random" (uniform), "unused5" (uniform without
    relation 5), "one" (every edge relation ``r - 1``), "distinct" (position in the graph's list modulo ``r``: every edge
    of a tile of up to ``r`` edges its own relation).  ``oor``: every seventh edge gets relation -1, every eleventh ``r``.
    Edge weights in [-1, 1) with every fifth one zero."""
    b = topo.batch(_graphs(kind, order, seed))
    rng = np.random.default_rng(100 + seed)
    n, e = int(b["row_splits"][-1]), len(b["flat"])
    k, u = ku
    if relations == "one":
        rel = np.full(e, r - 1, np.int64)
    elif relations == "distinct":
        rel = np.concatenate([np.arange(c) % r for c in np.diff(b["index_splits"])]).astype(np.int64)
    else:
        rel = rng.integers(0, r, size=e).astype(np.int64)
        if relations == "unused5":
            rel[rel == 5] = 6
    if oor:
        rel[::7] = -1
        rel[3::11] = r
    w = rng.uniform(-1.0, 1.0, size=(e, 1)).astype(np.float32)
    w[::5] = 0.0
    glorot = lambda *shape: (rng.uniform(-1, 1, size=shape) * np.sqrt(6.0 / (shape[-2] + shape[-1]))).astype(np.float32)
    small = lambda: rng.uniform(-0.1, 0.1, size=u).astype(np.float32) if bias else None
    b.update(nodes=rng.normal(size=(n, k)).astype(np.float32), rel=rel, edge_weights=w if weights else None, r=r, k=k, u=u,
             rows=n, act0=act0, act_m=act_m, act=act,
             params={"w0": glorot(k, u), "b0": small(), "kernel": glorot(r, k, u), "bias": small(),
                     "wg": glorot(r, k, u), "bg": small(), "wt": glorot(r, k, u), "bt": small()})
    return b


def kernel_restate(case, mode, dtype):
    """One block of ``mode`` ("rgcn" / "film") on a kernel case, numpy."""
    t = lambda a: None if a is None else torch.tensor(a, dtype=dtype)
    p = {key: t(v) for key, v in case["params"].items()}
    n = t(case["nodes"])
    if mode == "rgcn":
        out = rgcn_block(n, case["flat"], t(case["edge_weights"]), case["rel"], p, case["act0"], case["act"])
    else:
        out = film_block(n, case["flat"], case["rel"], p, case["act_m"], case["act"])
    return out.numpy()


def no_edge_rows(case, mode, dtype=torch.float64):
    """What a receiver without edges gets: RGCN ``act(act0(n W0 + b0))``, FiLM ``act(0)``."""
    t = lambda a: None if a is None else torch.tensor(a, dtype=dtype)
    if mode == "film":
        return activation(case["act"], torch.zeros((case["rows"], case["u"]), dtype=dtype)).numpy()
    h0 = t(case["nodes"]) @ t(case["params"]["w0"])
    if case["params"]["b0"] is not None:
        h0 = h0 + t(case["params"]["b0"])
    return activation(case["act"], activation(case["act0"], h0)).numpy()


# ------------------------------------------------------------------------------------------------------- model cases
MODEL_SIZES = (70, 1, 0, 21)     # a molecule of several tiles, a lone node, an empty graph, an aspirin-sized one
OUTPUT_MLP = {"use_bias": [True, True], "units": [16, 2], "activation": ["swish", "linear"]}


def model_batch(embed, seed, sizes=MODEL_SIZES, num_relations=20, features=32):
    """Ragged batch of ``sizes`` nodes with three unsorted random edges per node (self loops and duplicates happen; the lone
    node has three self loops), relations uniform in ``[0, num_relations)`` with one -1 and one ``num_relations``, edge
    weights in [-1, 1).  ``x``: float32 numbers for the embedding or ``features`` normal columns."""
    rng = np.random.default_rng(1000 + seed)
    graphs = [(n, np.stack([rng.integers(0, max(n, 1), size=3 * n), rng.integers(0, max(n, 1), size=3 * n)], axis=-1))
              for n in sizes]
    b = topo.batch(graphs)
    n, m = int(b["row_splits"][-1]), len(b["flat"])
    rel = rng.integers(0, num_relations, size=m).astype(np.int64)
    rel[4], rel[9] = -1, num_relations
    b.update(node_splits=b["row_splits"], edge_splits=b["index_splits"], edge_indices=b["indices"], edge_relations=rel,
             edge_weights=rng.uniform(-1.0, 1.0, size=(m, 1)).astype(np.float32),
             x=rng.integers(0, 95, size=n).astype(np.float32) if embed
             else rng.normal(size=(n, features)).astype(np.float32))
    return b


def model_cases(kind):
    """name -> (``make_model`` arguments, ``model_forward`` arguments, seed): depth 2 at the default widths with the
    embedding, at K = 32 != U = 128 on features with node output, and with ``num_bases`` / ``num_blocks`` kernels."""
    base = RGCN_INPUTS if kind == "rgcn" else FILM_INPUTS
    feat = [dict(s) for s in base]
    feat[0]["shape"] = (None, 32)
    rel = lambda u, **kw: dict({"units": u, "num_relations": 20}, **kw)
    mod = lambda u: {"units": u, "num_relations": 20, "activation": "sigmoid"}
    extra = (lambda u: {"dense_kwargs": {"units": u}}) if kind == "rgcn" else (lambda u: {"dense_modulation_kwargs": mod(u)})
    common = {"depth": 2, "output_mlp": OUTPUT_MLP}
    fwd = {"depth": 2, "embed": True}
    return {
        "default-graph": (dict(common, dense_relation_kwargs=rel(64), **extra(64)), dict(fwd), 11),
        "wide-node": (dict(common, inputs=feat, dense_relation_kwargs=rel(128), output_embedding="node",
                           output_to_tensor=False, **extra(128)),
                      dict(fwd, embed=False, output_embedding="node"), 12),
        "bases-blocks": (dict(common, dense_relation_kwargs=rel(64, num_bases=3, num_blocks=2), **extra(64)),
                         dict(fwd, num_bases=3, num_blocks=2), 13),
    }


RGCN_INPUTS = [{"shape": (None,), "name": "node_attributes", "dtype": "float32", "ragged": True},
               {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True},
               {"shape": (None, 1), "name": "edge_weights", "dtype": "float32", "ragged": True},
               {"shape": (None,), "name": "edge_relations", "dtype": "int64", "ragged": True}]
FILM_INPUTS = [RGCN_INPUTS[0], RGCN_INPUTS[1], RGCN_INPUTS[3]]
