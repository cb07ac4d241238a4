"""Per-graph torch-CPU restatement of PoolingTopK, UnPoolingTopK, AdjacencyPower and the Graph U-Net model, written from
the op sequence of kgcnn/layers/pool/topk.py and kgcnn/literature/Unet.py, in float32 or float64.

Where the reference leaves the result open, the rule is the one layers/pool/topk.py documents: kept nodes in ascending
``(score, index)`` (a stable sort on the score), duplicates in the adjacency unsupported.  ``AdjacencyPower`` is the
reference's own method on one graph: a dense ``A``, ``A @ A``, the mask ``> 1e-7``, row-major.

The segment mean of the convolution accumulates in edge order, as the engine's CSR walk does, and every product with a
weight matrix and every score is an explicit loop over the contracted axis in elementwise operations (``dense``): a
row's result then depends on the row alone - a BLAS kernel may round the same row differently at another position of
the matrix - so two nodes with the same neighbour list carry bit-equal rows and their scores tie exactly, in either
precision and on every machine.  ``trace`` (a list) collects per level and graph what the input conditions of the tests
are stated on.
"""
import numpy as np
import torch

EPS = 1e-7   # tf.keras.backend.epsilon()


def topk_counts(k, n):
    """``(nremove, nkeep)``: ``tf.math.round`` (half to even) of the float32 product (topk.py:96-98)."""
    rem = int(np.rint(np.float32(k) * np.float32(n)))
    rem = min(max(rem, 0), int(n))
    return rem, int(n) - rem


def dense(x, w, b=None):
    """``x @ w + b`` summed over the contracted axis in order, in elementwise operations: no row depends on its place."""
    acc = torch.zeros((x.shape[0], w.shape[1]), dtype=x.dtype)
    for c in range(w.shape[0]):
        acc = acc + x[:, c:c + 1] * w[c:c + 1, :]
    return acc if b is None else acc + b


def scores(x, p):
    """``sum_c (x_c p_c) / ||p||`` (topk.py:83-84), summed in order."""
    norm = torch.sqrt(torch.sum(p * p))
    s = torch.zeros(x.shape[0], dtype=x.dtype)
    for c in range(x.shape[1]):
        s = s + x[:, c] * p[0, c] / norm
    return s


def pooling_topk(x, edges, idx, p, k):
    """One graph: ``x (N, F)``, ``edges (M, Fe)``, ``idx (M, 2)`` numpy int64, ``p (1, F)``.  Returns ``x', edges', idx'
    (numpy), map_nodes (numpy), map_edges (numpy), s`` (the scores of all nodes)."""
    n = int(x.shape[0])
    s = scores(x, p)
    order = np.argsort(s.detach().numpy(), kind="stable")          # ascending (score, index); -0.0 == 0.0
    nremove, nkeep = topk_counts(k, n)
    kept = order[nremove:]
    gate = torch.sigmoid(s[kept]).unsqueeze(-1)
    x_new = x[kept] * gate
    new_id = -np.ones(n, dtype=np.int64)
    new_id[kept] = np.arange(nkeep)
    idx = np.asarray(idx, dtype=np.int64).reshape(-1, 2)
    alive = (new_id[idx[:, 0]] >= 0) & (new_id[idx[:, 1]] >= 0) if len(idx) else np.zeros(0, dtype=bool)
    pos = np.nonzero(alive)[0]
    new_idx = np.stack([new_id[idx[pos, 0]], new_id[idx[pos, 1]]], axis=1) if len(pos) else np.zeros((0, 2), np.int64)
    by_recv = np.argsort(new_idx[:, 0], kind="stable")
    pos = pos[by_recv]
    return x_new, edges[pos], new_idx[by_recv], kept.astype(np.int64), pos.astype(np.int64), s


def unpooling_topk(n_old, map_nodes, x_pool):
    out = torch.zeros((n_old,) + tuple(x_pool.shape[1:]), dtype=x_pool.dtype)
    if len(map_nodes):
        out = out.index_add(0, torch.from_numpy(np.asarray(map_nodes, dtype=np.int64)), x_pool)
    return out


def adjacency_dense(edges, idx, n):
    a = torch.zeros((n, n), dtype=edges.dtype)
    if len(idx):
        a[torch.from_numpy(idx[:, 0]), torch.from_numpy(idx[:, 1])] = edges[:, 0]
    return a


def adjacency_power(edges, idx, n, power=2, trace=None):
    """One graph: ``(edges' (M', 1), idx' (M', 2) numpy)``; ``trace`` gets ``(P, structural)``, the dense power and the
    positions a product can reach."""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1, 2)
    a = adjacency_dense(edges.detach(), idx, n)
    out = a
    pattern = (a != 0).to(torch.float64)
    reach = pattern
    for _ in range(power - 1):
        out = out @ a
        reach = ((reach @ pattern) > 0).to(torch.float64)
    if trace is not None:
        trace.append((out.numpy().copy(), reach.numpy() > 0))
    mask = (out > EPS).numpy()
    ii, kk = np.nonzero(mask)                                    # row-major
    return out[torch.from_numpy(ii), torch.from_numpy(kk)].unsqueeze(-1), np.stack([ii, kk], axis=1).astype(np.int64)


def segment_mean(rows, recv, n):
    """Mean of ``rows`` per receiver, each receiver's rows added in list order: round ``r`` adds the ``r``-th row of every
    receiver (distinct targets, so the order inside a round does not matter)."""
    recv = np.asarray(recv, dtype=np.int64)
    out = torch.zeros((n, rows.shape[1]), dtype=rows.dtype)
    cnt = np.bincount(recv, minlength=n) if len(recv) else np.zeros(n, dtype=np.int64)
    if len(recv):
        by_recv = np.argsort(recv, kind="stable")
        nth = np.empty(len(recv), dtype=np.int64)
        nth[by_recv] = np.arange(len(recv)) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        for r in range(int(nth.max()) + 1):
            pick = np.nonzero(nth == r)[0]
            out = out.index_add(0, torch.from_numpy(recv[pick]), rows[torch.from_numpy(pick)])
    return out / torch.from_numpy(np.maximum(cnt, 1)).to(rows.dtype).unsqueeze(-1)


def conv(x, idx, w, b, activation=torch.relu):
    """GatherNodesOutgoing -> Dense -> PoolingLocalEdges(mean) -> Activation (Unet.py:116-119), the Dense per edge row."""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1, 2)
    eu = dense(x[torch.from_numpy(idx[:, 1])], w, b)
    return activation(segment_mean(eu, idx[:, 0], int(x.shape[0])))


def unet_forward(weights, batch, depth=4, k=0.3, use_reconnect=True, output_embedding="graph", embed_nodes=False,
                 embed_edges=False, dtype=torch.float32, trace=None):
    """The model on ``batch`` (``nodes``, ``edges``, ``edge_indices``, ``node_splits``, ``edge_splits`` as numpy; nodes /
    edges are numbers for an embedding input, feature rows otherwise) with ``weights`` in ``model.weights`` order (torch
    tensors of ``dtype``, so that autograd reaches them).  Returns ``(G, L)`` for ``"graph"`` and the concatenated node
    rows ``(N, L)`` for ``"node"``.  ``trace``: list receiving one dict per graph with the per-level ``scores`` (all
    nodes of the level), ``kept`` (input ids) and ``powers`` (``adjacency_power``'s trace)."""
    w = list(weights)
    emb_n = w.pop(0) if embed_nodes else None
    emb_e = w.pop(0) if embed_edges else None
    w0, b0 = w.pop(0), w.pop(0)
    down = [(w.pop(0), w.pop(0), w.pop(0)) for _ in range(depth)]
    up = [(w.pop(0), w.pop(0)) for _ in range(depth)]
    wm0, bm0, wm1 = w
    ns, es = batch["node_splits"], batch["edge_splits"]
    outs = []
    for g in range(len(ns) - 1):
        xn = batch["nodes"][ns[g]:ns[g + 1]]
        xe = batch["edges"][es[g]:es[g + 1]]
        idx = np.asarray(batch["edge_indices"][es[g]:es[g + 1]], dtype=np.int64)
        x = emb_n[torch.from_numpy(xn.astype(np.int64))] if embed_nodes else torch.from_numpy(xn).to(dtype)
        e = emb_e[torch.from_numpy(xe.astype(np.int64))] if embed_edges else torch.from_numpy(xe).to(dtype)
        e = e.detach()
        x = dense(x, w0, b0)
        graphs, maps = [(x, e, idx)], []
        rec = {"scores": [], "kept": [], "powers": []}
        for wd, bd, p in down:
            x, e, idx = graphs[-1]
            x = conv(x, idx, wd, bd)
            if use_reconnect:
                e, idx = adjacency_power(e, idx, int(x.shape[0]), 2, rec["powers"])
            x_new, e_new, idx_new, map_n, map_e, s = pooling_topk(x, e, idx, p, k)
            rec["scores"].append(s.detach().numpy().copy())
            rec["kept"].append(map_n.copy())
            graphs.append((x_new, e_new, idx_new))
            maps.append(map_n)
        x = graphs[-1][0]
        for level, (wu, bu) in zip(range(depth, 0, -1), up):
            x_old, _, idx_old = graphs[level - 1]
            x = unpooling_topk(int(x_old.shape[0]), maps[level - 1], x) + x_old
            x = conv(x, idx_old, wu, bu)
        if trace is not None:
            trace.append(rec)
        if output_embedding == "graph":
            pooled = x.mean(dim=0, keepdim=True) if x.shape[0] else torch.zeros((1, x.shape[1]), dtype=dtype)
            outs.append(torch.sigmoid(dense(torch.relu(dense(pooled, wm0, bm0)), wm1)))
        else:
            outs.append(torch.sigmoid(dense(torch.relu(dense(x, wm0, bm0)), wm1)))
    return torch.cat(outs, dim=0)


def check_input_conditions(trace32, trace64, margin=1e-4):
    """The conditions under which the reference alone is unambiguous (asserted by the tests on their seeds):

    * float64: every ``A^n`` entry on a structurally possible position differs from 1e-7 by at least ``margin``;
    * at every level, every gap between adjacent sorted scores of a graph is exactly zero in both precisions or at least
      ``margin * max|score|`` (in both);
    * the float32 restatement keeps the same nodes as the float64 one.

    Returns ``(smallest threshold margin, smallest non-zero relative gap, number of exact ties)``."""
    thr, gap_min, ties = np.inf, np.inf, 0
    for r32, r64 in zip(trace32, trace64):
        for power, reach in r64["powers"]:
            if reach.any():
                thr = min(thr, float(np.min(np.abs(power[reach] - EPS))))
        for s32, s64, k32, k64 in zip(r32["scores"], r64["scores"], r32["kept"], r64["kept"]):
            assert np.array_equal(k32, k64), "float32 and float64 keep different nodes"
            if len(s64) < 2:
                continue
            order = np.argsort(s64, kind="stable")
            assert np.array_equal(order, np.argsort(s32, kind="stable")), "float32 and float64 order the scores differently"
            for s in (s32.astype(np.float64), s64):
                gaps = np.diff(s[order])
                scale = float(np.max(np.abs(s)))
                nonzero = gaps[gaps != 0]
                if nonzero.size:
                    gap_min = min(gap_min, float(nonzero.min()) / max(scale, 1e-30))
            z32, z64 = np.diff(s32[order]) == 0, np.diff(s64[order]) == 0
            assert np.array_equal(z32, z64), "a score tie is exact in one precision only"
            ties += int(z64.sum())
    assert thr >= margin, "an A^n entry is within %.3g of the threshold" % thr
    assert gap_min >= margin, "adjacent scores differ by %.3g of the scale: neither a tie nor a clear gap" % gap_min
    return thr, gap_min, ties
