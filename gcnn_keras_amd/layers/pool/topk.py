"""Top-k pooling layers (mirror of kgcnn/layers/pool/topk.py) on the HIP engine: ``PoolingTopK`` (gPool of Gao & Ji),
``UnPoolingTopK`` and ``AdjacencyPower``, with the reference's class names, constructor arguments, input / output lists
and ``get_config`` keys.  The kernels are csrc/mp_topk.hip; nothing here forms the reference's ``(batch*M, 2, removed)``
mask or its padded ``(batch, Nmax, Nmax)`` adjacency.

All three honour ``node_indexing`` ``"sample"`` (ids local to the graph, the default) and ``"batch"`` (batch-wide ids).

Sizes are data dependent: ``PoolingTopK`` reads the pooled edge splits back once per call and ``AdjacencyPower`` the new
edge splits once per product; the pooled node count is a function of the row lengths alone and is computed on the host.
The index tensors these layers return carry a ready index plan (shifted columns and receiver CSR), so the layers behind
them launch no index preparation.

Training.  The selection (which nodes and edges survive, in which order) is a constant of the tape.  The values are
differentiable: in grad mode ``PoolingTopK`` gathers the kept rows, takes the score as a ``Dense`` on ``p / ||p||`` and
gates with ``Activation`` and ``Binary`` ops, ``UnPoolingTopK`` scatters with the adjoint of the row gather; outside a
tape both take the fused launches.  ``AdjacencyPower``'s edge values carry no gradient (see there).
"""
import numpy as np
import torch

from ... import _ffi
from ...ragged import IndexPlan, RaggedTensor
from ..base import GraphBaseLayer

KERAS_EPSILON = 1e-7   # tf.keras.backend.epsilon(), the threshold of AdjacencyPower (topk.py:367)


def topk_counts(k, row_lengths):
    """``(nremove, nkeep)`` per graph for node counts ``row_lengths`` (host integers): ``nremove = rint(float32(k) *
    float32(N_g))``, half to even (``tf.math.round`` on floatx, topk.py:96), clipped to ``[0, N_g]``."""
    lengths = np.asarray(row_lengths, dtype=np.int64)
    rem = np.rint(np.float32(k) * lengths.astype(np.float32)).astype(np.int64)
    rem = np.clip(rem, 0, lengths)
    return rem, lengths - rem


class _TopKBase(GraphBaseLayer):
    """``GraphBaseLayer`` that also takes ``node_indexing="batch"`` (the base class serves "sample" only)."""

    def __init__(self, node_indexing="sample", **kwargs):
        if node_indexing not in ("sample", "batch"):
            raise ValueError("node_indexing must be 'sample' or 'batch', got %r" % (node_indexing,))
        super().__init__(**kwargs)
        self.node_indexing = node_indexing
        self._kgcnn_info["node_indexing"] = node_indexing

    @property
    def _batch(self):
        return 1 if self.node_indexing == "batch" else 0

    def _plan(self, idx, nodes):
        """Index plan of ``idx`` against ``nodes``: the attached one, else built from the values in this layer's
        ``node_indexing`` form."""
        key = (nodes.row_splits.data_ptr(), int(nodes.values.shape[0]))
        plan = idx._plans.get(key)
        if plan is not None or not self._batch:
            return plan if plan is not None else idx.index_plan(nodes)
        n = int(nodes.values.shape[0])
        cols = idx.values.t().clamp(0, max(n - 1, 0)).to(torch.int32).contiguous()
        if cols.shape[1] == 0:
            cols = torch.zeros((cols.shape[0], 1), dtype=torch.int32, device=cols.device)
        plan = IndexPlan.from_prepared(idx, nodes, cols,
                                       flags=_ffi.MP_FLAG_UNSORTED_COL0 | _ffi.MP_FLAG_UNSORTED_COL1)
        idx._plans[key] = plan
        return plan


def _workspace(n, device):
    nbytes = _ffi.workspace_bytes("mp_topk_workspace_bytes", int(n))
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device), nbytes


def _ragged(values, splits, splits_host):
    out = RaggedTensor(values, splits)
    out._splits_host = splits_host
    return out


def _selection_plan(map_ragged, target, cols):
    """Plan of a ``(Nk, 1)`` map whose shifted int32 column ``cols`` (1, max(Nk, 1)) is known: unsorted, CSR on demand
    (the reverse rules ask for it)."""
    as_idx = RaggedTensor(map_ragged.values.view(-1, 1), map_ragged.row_splits)
    return IndexPlan.from_prepared(as_idx, target, cols, flags=_ffi.MP_FLAG_UNSORTED_COL0 | _ffi.MP_FLAG_UNSORTED_COL1)


class PoolingTopK(_TopKBase):
    r"""Learnable top-k node pooling with gate (kgcnn/layers/pool/topk.py:9-211).

    ``call([nodes (batch,[N],F), edges (batch,[M],Fe), edge_indices (batch,[M],2)])`` returns ``([nodes', edges',
    edge_indices'], [map_nodes, map_edges])``.  Weight ``score`` of shape ``(1, F)``.

    * score :math:`s_i = \sum_c (n_{ic} p_c) / \lVert p \rVert`;
    * per graph ``nremove = round_half_to_even(float32(k) * float32(N_g))`` nodes go, ``nkeep = N_g - nremove`` stay
      (:func:`topk_counts`; k = 0.3: 5 nodes lose 2, 15 lose 4);
    * the kept nodes are the ``nkeep`` highest scores, **in ascending score inside the graph** (the reference's
      ``sort12`` order, not the input order).  The reference's first argsort is unstable, so its order among equal scores
      is undefined; here equal scores order by ascending input index, i.e. the sort key is ``(s_i, i)``.  Scores
      compare as floats (``-0.0 == 0.0``).  Non-finite scores are not supported;
    * ``nodes' = n_i * sigmoid(s_i)``; ``map_nodes`` the old index of every kept node;
    * kept edges have both ends kept, are re-indexed to the new node numbers and ordered by new ``edge_indices[:, 0]``,
      stable in the old edge order; ``edges'`` their feature rows, ``map_edges`` their old position in the graph's list;
    * graphs without nodes, without kept nodes or without surviving edges give empty rows, trailing ones included.

    Launches outside a tape: the selection (4 kernels in one entry), the edge count and the edge fill, after the old edge
    list's receiver CSR; one host read (the pooled edge splits).  In grad mode the selection runs the same way and the
    values are recomputed by ops with reverse rules; there the score is ``n @ (p / ||p||)``, which rounds differently from
    the selection's ``sum(n p / ||p||)`` in the last bits."""

    weight_gradients = True   # the score weight is on the tape in grad mode (tests/test_gpu_unet.py)

    def __init__(self, k=0.1, kernel_initializer="glorot_uniform", kernel_regularizer=None, kernel_constraint=None,
                 **kwargs):
        super().__init__(**kwargs)
        self.k = k
        self.kernel_initializer = kernel_initializer
        self.kernel_regularizer = kernel_regularizer
        self.kernel_constraint = kernel_constraint
        self.units_p = None
        self.kernel_p = None

    def build(self, input_shape):
        super().build(input_shape)
        self.units_p = int(input_shape[0][-1])
        self.kernel_p = self.add_weight("score", (1, self.units_p), self.kernel_initializer)

    # -- the selection: a constant of the tape ---------------------------------------------------------------------
    def _select(self, nodes):
        x = nodes.values.detach().contiguous()
        if x.dtype != torch.float32 or x.dim() != 2:
            raise TypeError("PoolingTopK expects float32 nodes of shape (batch, [N], F)")
        n, f, g, dev = int(x.shape[0]), int(x.shape[1]), nodes.nrows(), x.device
        if not 0.0 <= float(self.k) <= 1.0:
            raise ValueError("PoolingTopK: k = %r is outside [0, 1]" % (self.k,))
        _, nkeep = topk_counts(self.k, np.diff(nodes.row_splits_host()))
        new_host = np.concatenate([[0], np.cumsum(nkeep)]).astype(np.int64)
        nk = int(new_host[-1])
        sel = {"N": n, "Nk": nk, "new_splits_host": new_host,
               "score": torch.empty(n, dtype=torch.float32, device=dev),
               "new_splits": torch.zeros(g + 1, dtype=torch.int64, device=dev),
               "out": torch.empty((nk, f), dtype=torch.float32, device=dev),
               "map_nodes": torch.empty(nk, dtype=torch.int64, device=dev),
               "map_global": torch.zeros((1, max(nk, 1)), dtype=torch.int32, device=dev),
               "old2new": torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev)}
        if g > 0:
            ws, nbytes = _workspace(g, dev)
            _ffi.call("mp_topk_select_f32", _ffi.ptr(x), n, f, _ffi.ptr(self.kernel_p.detach().contiguous()),
                      _ffi.ptr(nodes.row_splits), g, float(self.k), nk, self._batch, _ffi.ptr(sel["score"]),
                      _ffi.ptr(sel["new_splits"]), _ffi.ptr(sel["out"]), _ffi.ptr(sel["map_nodes"]),
                      _ffi.ptr(sel["map_global"]), _ffi.ptr(sel["old2new"]), _ffi.ptr(ws), nbytes, _ffi.stream())
        return sel

    def _induced_edges(self, nodes, edges, idx, sel):
        ev = edges.values.detach().contiguous()
        if ev.dtype != torch.float32:
            raise TypeError("PoolingTopK expects float32 edges, got %s" % ev.dtype)
        m, g, dev = int(ev.shape[0]), nodes.nrows(), ev.device
        fe = 1
        for d in ev.shape[1:]:
            fe *= int(d)
        ev2 = ev.view(m, fe)
        n, nk = sel["N"], sel["Nk"]
        plan = self._plan(idx, nodes)
        if plan.K != 2:
            raise ValueError("PoolingTopK expects edge indices of shape (batch, [M], 2)")
        if plan.M != m or edges.nrows() != g or idx.nrows() != g:
            raise ValueError("PoolingTopK: nodes, edges and edge indices disagree in batch size or edge count")
        if self.ragged_validate:
            plan.validate()
        ptr0, perm0, _ = plan.csr(0, assume_sorted=self.is_sorted)
        send = plan.col(1).contiguous()
        off = torch.zeros(nk + 1, dtype=torch.int64, device=dev)
        esplits = torch.zeros(g + 1, dtype=torch.int64, device=dev)
        if g > 0:
            ws, nbytes = _workspace(nk, dev)
            _ffi.call("mp_topk_edges_count_i32", _ffi.ptr(ptr0), _ffi.ptr(perm0), _ffi.ptr(send), m, n,
                      _ffi.ptr(sel["map_global"]), _ffi.ptr(sel["old2new"]), nk, _ffi.ptr(sel["new_splits"]), g,
                      _ffi.ptr(off), _ffi.ptr(esplits), _ffi.ptr(ws), nbytes, _ffi.stream())
        esplits_host = esplits.cpu().numpy()   # data-dependent output size: the one host read of this layer
        mk = int(esplits_host[-1])
        out = {"Mk": mk, "splits": esplits, "splits_host": esplits_host,
               "edges": torch.empty((mk,) + tuple(ev.shape[1:]), dtype=torch.float32, device=dev),
               "idx": torch.empty((mk, 2), dtype=torch.int64, device=dev),
               "map_edges": torch.empty(mk, dtype=torch.int64, device=dev),
               "map_global": torch.zeros((1, max(mk, 1)), dtype=torch.int32, device=dev),
               "cols": torch.zeros((2, max(mk, 1)), dtype=torch.int32, device=dev),
               "ptr": torch.zeros(nk + 1, dtype=torch.int32, device=dev),
               "old2new": torch.full((max(m, 1),), -1, dtype=torch.int32, device=dev)}
        _ffi.call("mp_topk_edges_fill_f32", _ffi.ptr(ptr0), _ffi.ptr(perm0), _ffi.ptr(send), m, n,
                  _ffi.ptr(sel["map_global"]), _ffi.ptr(sel["old2new"]), nk, _ffi.ptr(sel["new_splits"]),
                  _ffi.ptr(edges.row_splits), g, _ffi.ptr(off), mk, _ffi.ptr(ev2), fe, self._batch,
                  _ffi.ptr(out["edges"]), _ffi.ptr(out["idx"]), _ffi.ptr(out["map_edges"]), _ffi.ptr(out["map_global"]),
                  _ffi.ptr(out["cols"]), _ffi.ptr(out["ptr"]), _ffi.ptr(out["old2new"]) if m > 0 else None,
                  _ffi.stream())
        return out

    def call(self, inputs, **kwargs):
        from ...autograd import needs_grad
        nodes, edges, idx = self.assert_ragged_input_rank(list(inputs))
        _ffi.require_device(nodes.values, edges.values, idx.values, self.kernel_p)
        sel = self._select(nodes)
        ed = self._induced_edges(nodes, edges, idx, sel)
        map_nodes = _ragged(sel["map_nodes"], sel["new_splits"], sel["new_splits_host"])
        map_edges = _ragged(ed["map_edges"], ed["splits"], ed["splits_host"])
        # what UnPoolingTopK needs beyond the maps' values: the inverse tables (fused launch) and the plans (reverse rule)
        map_nodes._topk = {"old2new": sel["old2new"], "plan": _selection_plan(map_nodes, nodes, sel["map_global"])}
        map_edges._topk = {"old2new": ed["old2new"], "plan": _selection_plan(map_edges, edges, ed["map_global"])}
        node_vals, edge_vals = sel["out"], ed["edges"]
        if needs_grad(nodes.values, self.kernel_p):
            node_vals = self._gated_rows_on_tape(nodes.values, map_nodes._topk["plan"])
        if needs_grad(edges.values):
            from ..gather import gather_rows
            edge_vals = gather_rows(edges.values, map_edges._topk["plan"], [0])[:, 0]
        nodes_out = _ragged(node_vals, sel["new_splits"], sel["new_splits_host"])
        edges_out = _ragged(edge_vals, ed["splits"], ed["splits_host"])
        idx_out = _ragged(ed["idx"], ed["splits"], ed["splits_host"])
        # column 0 (the new receiver) is sorted by construction, column 1 is not claimed
        idx_out.attach_plan(nodes_out, IndexPlan.from_prepared(idx_out, nodes_out, ed["cols"], ed["ptr"]))
        return [nodes_out, edges_out, idx_out], [map_nodes, map_edges]

    def _gated_rows_on_tape(self, x, plan):
        """``x[kept] * sigmoid(x[kept] @ (p / ||p||))`` from ops with reverse rules (topk.py:83-84, 107-116)."""
        from ..gather import gather_rows
        from ..geom import EuclideanNorm
        from ..modules import binary_values, dense_values
        from ...ops.activ import apply_activation
        inv = EuclideanNorm._compute_euclidean_norm(self.kernel_p, axis=-1, keepdims=True, invert_norm=True)
        w = binary_values(_ffi.MP_MUL, self.kernel_p, inv)                      # (1, F)
        kept = gather_rows(x, plan, [0])[:, 0]                                  # (Nk, F)
        s = dense_values(kept, w.reshape(self.units_p, 1), None)                # (Nk, 1)
        return binary_values(_ffi.MP_MUL, kept, apply_activation("sigmoid", s))

    def get_config(self):
        config = super().get_config()
        config.update({"k": self.k, "kernel_initializer": self.kernel_initializer,
                       "kernel_regularizer": self.kernel_regularizer, "kernel_constraint": self.kernel_constraint})
        return config


class UnPoolingTopK(_TopKBase):
    """Reverse of :class:`PoolingTopK` (kgcnn/layers/pool/topk.py:215-292).

    ``call([node, edge, edge_indices, map_node, map_edge, node_pool, edge_pool, edge_indices_pool])`` returns ``[nodes,
    edges, edge_indices]``: zeros of the old node (edge) count and the pooled width with the pooled rows written at
    ``map_node`` (``map_edge``); the old ``edge_indices`` pass through.  One launch per tensor with maps that come from
    ``PoolingTopK`` (they carry the inverse table); other maps cost one more to invert.  ``call_with_skip`` also adds a
    skip tensor in the same launch (``UnPoolingTopK`` + ``LazyAdd`` of the model)."""

    weight_gradients = True   # layers/base.py: no weight of this layer is left off the tape

    def _tables(self, map_ragged, target):
        """``(old2new, plan)`` of a map against the old tensor ``target``."""
        cached = getattr(map_ragged, "_topk", None)
        if cached is not None and int(cached["old2new"].shape[0]) == max(int(target.values.shape[0]), 1):
            return cached["old2new"], cached["plan"]
        if map_ragged.values.dtype != torch.int64 or map_ragged.values.dim() != 1:
            raise TypeError("UnPoolingTopK expects int64 maps of shape (batch, [Nk])")
        n, nk, dev = int(target.values.shape[0]), int(map_ragged.values.shape[0]), target.values.device
        old2new = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev)
        _ffi.call("mp_topk_invert_map_i64", _ffi.ptr(map_ragged.values.contiguous()), nk, _ffi.ptr(map_ragged.row_splits),
                  _ffi.ptr(target.row_splits), map_ragged.nrows(), self._batch, n, _ffi.ptr(old2new), _ffi.stream())
        as_idx = RaggedTensor(map_ragged.values.view(-1, 1), map_ragged.row_splits)
        plan = self._plan(as_idx, target)
        map_ragged._topk = {"old2new": old2new, "plan": plan}
        return old2new, plan

    def _scatter(self, pooled, map_ragged, target, skip=None):
        from ...autograd import GatherRowsAdjoint, needs_grad
        pv = pooled.values
        if pv.dtype != torch.float32:
            raise TypeError("UnPoolingTopK expects float32 values, got %s" % pv.dtype)
        n, nk = int(target.values.shape[0]), int(pv.shape[0])
        if int(map_ragged.values.shape[0]) != nk:
            raise ValueError("UnPoolingTopK: map and pooled tensor differ in length")
        old2new, plan = self._tables(map_ragged, target)
        shape = (n,) + tuple(pv.shape[1:])
        if needs_grad(pv, skip):
            out = GatherRowsAdjoint.apply(pv.contiguous().unsqueeze(1), plan, (0,), shape)
            if skip is not None:
                from ..modules import binary_values
                out = binary_values(_ffi.MP_ADD, out, skip)
            return out
        width = 1
        for d in pv.shape[1:]:
            width *= int(d)
        out = torch.empty(shape, dtype=torch.float32, device=pv.device)
        if skip is not None and tuple(skip.shape) != shape:
            raise ValueError("UnPoolingTopK: skip tensor of shape %s, expected %s" % (tuple(skip.shape), shape))
        _ffi.call("mp_topk_unpool_f32", _ffi.ptr(pv.contiguous()), nk, max(width, 1), _ffi.ptr(old2new), n,
                  _ffi.ptr(skip.contiguous()) if skip is not None else None, _ffi.ptr(out), _ffi.stream())
        return out

    def call(self, inputs, **kwargs):
        return self.call_with_skip(inputs, None)

    def call_with_skip(self, inputs, skip, with_edges=True):
        """``call`` with ``skip`` (ragged like the old nodes, of the pooled width) added to the node output.  Without
        ``with_edges`` the edge output is not computed and the old edge tensor is returned in its place."""
        node, edge, edge_indices, map_node, map_edge, node_pool, edge_pool, _ = self.assert_ragged_input_rank(list(inputs))
        _ffi.require_device(node.values, node_pool.values, edge_pool.values)
        out_node = self._scatter(node_pool, map_node, node, None if skip is None else skip.values)
        if not with_edges:
            return [node.with_values(out_node), edge, edge_indices]
        out_edge = self._scatter(edge_pool, map_edge, edge)
        return [node.with_values(out_node), edge.with_values(out_edge), edge_indices]


class AdjacencyPower(_TopKBase):
    """Powers of the adjacency matrix on the edge list (kgcnn/layers/pool/topk.py:296-397).

    ``call([nodes, edges, edge_indices])`` returns ``[edges', edge_indices']``.  Per graph ``A[i, j] = edges[e, 0]`` for
    ``edge_indices[e] = (i, j)`` (column 0 of the features only, as in the reference), ``P = A^n``, and every entry
    ``P[i, k] > 1e-7`` (the Keras epsilon) becomes an edge ``(i, k)`` of width 1, in row-major order (``i``, then ``k``
    ascending).  Negative entries and entries that cancel to below epsilon are dropped.  ``n = 1`` is the thresholding
    alone; ``n > 2`` applies the product ``n - 1`` times, the intermediate powers keeping every non-zero entry.

    Duplicate ``(i, j)`` pairs are undefined in the reference (``tensor_scatter_nd_update``) and not supported here; they
    are not checked for.  No dense matrix is formed: a product is two launches around a prefix sum and one host read of
    the new edge splits, and graphs of any size are served (rows accumulate in LDS over column ranges).

    The output values carry no gradient: the entries are a thresholded function of the input weights and nothing behind
    this layer in Graph U-Net reads them.  An edge input that requires grad raises ``NotImplementedError``."""

    weight_gradients = True   # layers/base.py: no weights

    def __init__(self, n=2, **kwargs):
        super().__init__(**kwargs)
        self.n = n
        if int(n) != n or n < 1:
            raise ValueError("AdjacencyPower: n must be a positive integer, got %r" % (n,))

    def _product(self, left, right, nodes, final):
        """One ``L . R`` (``right is None``: ``R`` = identity) -> the operand dict of the product."""
        n, g, dev = int(nodes.values.shape[0]), nodes.nrows(), nodes.values.device
        off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        esplits = torch.zeros(g + 1, dtype=torch.int64, device=dev)
        r = right or {"ptr": None, "perm": None, "col": None, "val": None, "ld": 1, "M": 0}
        operands = (_ffi.ptr(left["ptr"]), _ffi.ptr(left["perm"]), _ffi.ptr(left["col"]), _ffi.ptr(left["val"]),
                    left["ld"], left["M"], _ffi.ptr(r["ptr"]), _ffi.ptr(r["perm"]), _ffi.ptr(r["col"]), _ffi.ptr(r["val"]),
                    r["ld"], r["M"], n, _ffi.ptr(nodes.row_splits), g, float(KERAS_EPSILON), 0 if final else 1)
        if g > 0:
            ws, nbytes = _workspace(n, dev)
            _ffi.call("mp_adjacency_product_count_f32", *operands, _ffi.ptr(off), _ffi.ptr(esplits), _ffi.ptr(ws),
                      nbytes, _ffi.stream())
        esplits_host = esplits.cpu().numpy()   # data-dependent output size: one host read per product
        mo = int(esplits_host[-1])
        vals = torch.empty((mo, 1), dtype=torch.float32, device=dev)
        idx = torch.empty((mo, 2), dtype=torch.int64, device=dev)
        cols = torch.zeros((2, max(mo, 1)), dtype=torch.int32, device=dev)
        ptr = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        _ffi.call("mp_adjacency_product_fill_f32", *operands, _ffi.ptr(off), mo, self._batch, _ffi.ptr(vals),
                  _ffi.ptr(idx), _ffi.ptr(cols), _ffi.ptr(ptr), _ffi.stream())
        return {"ptr": ptr, "perm": None, "col": cols[1, :mo].contiguous() if mo else cols[1, :1], "val": vals, "ld": 1,
                "M": mo, "idx": idx, "cols": cols, "splits": esplits, "splits_host": esplits_host}

    def call(self, inputs, **kwargs):
        from ...autograd import needs_grad
        nodes, edges, idx = self.assert_ragged_input_rank(list(inputs))
        _ffi.require_device(nodes.values, edges.values, idx.values)
        if needs_grad(edges.values):
            raise NotImplementedError("AdjacencyPower: the edge values carry no gradient (the output is a thresholded "
                                      "function of them); detach the edge input")
        ev = edges.values.contiguous()
        if ev.dtype != torch.float32 or ev.dim() != 2 or int(ev.shape[1]) < 1:
            raise TypeError("AdjacencyPower expects float32 edges of shape (batch, [M], Fe), Fe >= 1")
        plan = self._plan(idx, nodes)
        if plan.K != 2:
            raise ValueError("AdjacencyPower expects edge indices of shape (batch, [M], 2)")
        if plan.M != int(ev.shape[0]) or edges.nrows() != nodes.nrows() or idx.nrows() != nodes.nrows():
            raise ValueError("AdjacencyPower: nodes, edges and edge indices disagree in batch size or edge count")
        if self.ragged_validate:
            plan.validate()
        ptr0, perm0, _ = plan.csr(0, assume_sorted=self.is_sorted)
        a = {"ptr": ptr0, "perm": perm0, "col": plan.col(1).contiguous(), "val": ev, "ld": int(ev.shape[1]),
             "M": int(ev.shape[0])}
        steps = int(self.n) - 1
        out = self._product(a, None, nodes, True) if steps == 0 else a
        for t in range(steps):
            out = self._product(out, a, nodes, t == steps - 1)
        edges_out = _ragged(out["val"], out["splits"], out["splits_host"])
        idx_out = _ragged(out["idx"], out["splits"], out["splits_host"])
        # row-major by construction: column 0 is sorted, the product's row CSR is the receiver CSR
        idx_out.attach_plan(nodes, IndexPlan.from_prepared(idx_out, nodes, out["cols"], out["ptr"]))
        return [edges_out, idx_out]

    def get_config(self):
        config = super().get_config()
        config.update({"n": self.n})
        return config
