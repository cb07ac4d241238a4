"""On-GPU ``SetRange``, ``SetAngle`` and ``SetRangePeriodic`` (mirrors of kgcnn/graph/preprocessor.py:255-441 for a
ragged batch resident in HBM).

The reference runs ``define_adjacency_from_distance`` (kgcnn/graph/adj.py:537-593) per molecule in NumPy on the host
and re-uploads the edge lists; here the whole batch goes through two kernels around one prefix sum
(csrc/mp_radius.hip).  Same rule: ``dist < max_distance`` AND among the ``max_neighbours + 1`` nearest entries of the
row (exclusive mode), no self loops, row-major ``(i, j)`` order - hence receiver-sorted output.

``SetAngle`` is the second half of the geometry pre-step: the reference loops over the edges of one molecule in Python
(``get_angle_indices``, kgcnn/graph/adj.py:300-385); here the angle list of the whole batch comes from a count and a
fill kernel around one prefix sum (csrc/mp_angle.hip), walking the CSR buckets the edge list's index plan already has.

``SetRangePeriodic`` is ``SetRange`` for periodic cells: senders are atoms in periodic images of the cell
(``range_neighbour_lattice``, kgcnn/graph/geom.py:172-368); one wave per receiver enumerates the exact image box of every
sender and sorts its hits in LDS (csrc/mp_lattice.hip).
"""
import torch

from .. import _ffi
from ..ragged import RaggedTensor


class SetRange:

    def __init__(self, *, range_indices: str = "range_indices", node_coordinates: str = "node_coordinates",
                 range_attributes: str = "range_attributes", max_distance: float = 4.0, max_neighbours: int = 15,
                 do_invert_distance: bool = False, self_loops: bool = False, exclusive: bool = True, name="set_range",
                 overwrite: bool = True, **kwargs):
        if self_loops or not exclusive or do_invert_distance:
            raise NotImplementedError("on-GPU SetRange covers the configuration the training scripts use: exclusive, "
                                      "no self loops, plain distances")
        self.name = name
        self._config_kwargs = {"node_coordinates": node_coordinates, "range_indices": range_indices,
                               "range_attributes": range_attributes, "max_distance": max_distance,
                               "max_neighbours": max_neighbours, "do_invert_distance": do_invert_distance,
                               "self_loops": self_loops, "exclusive": exclusive, "overwrite": overwrite}
        self.max_distance = max_distance
        self.max_neighbours = max_neighbours

    def get_config(self):
        return {"name": self.name, **self._config_kwargs}

    @property
    def produces(self):
        """Property names this preprocessor adds when used on a dict of packed tensors (MD driver)."""
        return (self._config_kwargs["range_indices"], self._config_kwargs["range_attributes"])

    def __call__(self, node_coordinates):
        if isinstance(node_coordinates, dict):  # dict of packed device tensors -> dict of the new properties
            idx, attr = self._run(node_coordinates[self._config_kwargs["node_coordinates"]])
            return {self._config_kwargs["range_indices"]: idx, self._config_kwargs["range_attributes"]: attr}
        return self._run(node_coordinates)

    def count_edges(self, node_coordinates: RaggedTensor):
        """Pass 1 alone: the int64 edge row_splits ``(G+1)`` the rule produces for this batch (device tensor).  Used to
        balance graph shards by edge count before any edge list exists (gcnn_keras_amd/sharding.py)."""
        xyz = node_coordinates.values.contiguous()
        _ffi.require_device(xyz, node_coordinates.row_splits)
        n, g = int(xyz.shape[0]), node_coordinates.nrows()
        md = -1.0 if self.max_distance is None else float(self.max_distance)
        mn = -1 if self.max_neighbours is None else int(min(self.max_neighbours, 2 ** 30))
        nbytes = _ffi.workspace_bytes("mp_radius_graph_workspace_bytes", n)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=xyz.device)
        node_ptr = torch.empty(n + 1, dtype=torch.int32, device=xyz.device)
        edge_splits = torch.empty(g + 1, dtype=torch.int64, device=xyz.device)
        _ffi.call("mp_radius_graph_count_f32", _ffi.ptr(xyz), _ffi.ptr(node_coordinates.row_splits), g, n, md, mn,
                  _ffi.ptr(node_ptr), _ffi.ptr(edge_splits), _ffi.ptr(ws), nbytes, _ffi.stream())
        return edge_splits

    def _run(self, node_coordinates: RaggedTensor):
        """``node_coordinates``: ragged ``(batch, [N], 3)`` float32.  Returns ``(range_indices, range_attributes)``:
        ragged ``(batch, [M], 2)`` int64 sample indices and ragged ``(batch, [M], 1)`` distances; the returned index
        tensor carries a ready index plan (int32 ids + receiver CSR), so the first gather / pooling costs nothing."""
        xyz = node_coordinates.values.contiguous()
        _ffi.require_device(xyz, node_coordinates.row_splits)
        n, g = int(xyz.shape[0]), node_coordinates.nrows()
        dev = xyz.device
        md = -1.0 if self.max_distance is None else float(self.max_distance)
        mn = -1 if self.max_neighbours is None else int(min(self.max_neighbours, 2 ** 30))
        nbytes = _ffi.workspace_bytes("mp_radius_graph_workspace_bytes", n)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        node_ptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
        edge_splits = torch.empty(g + 1, dtype=torch.int64, device=dev)
        _ffi.call("mp_radius_graph_count_f32", _ffi.ptr(xyz), _ffi.ptr(node_coordinates.row_splits), g, n, md, mn,
                  _ffi.ptr(node_ptr), _ffi.ptr(edge_splits), _ffi.ptr(ws), nbytes, _ffi.stream())
        m = int(node_ptr[-1].item())  # the output size is data dependent: one host read, as in the reference pipeline
        idx = torch.empty((m, 2), dtype=torch.int64, device=dev)
        cols = torch.empty((2, max(m, 1)), dtype=torch.int32, device=dev)
        recv, send = cols[0], cols[1]
        dist = torch.empty((m, 1), dtype=torch.float32, device=dev)
        _ffi.call("mp_radius_graph_fill_f32", _ffi.ptr(xyz), _ffi.ptr(node_coordinates.row_splits), g, n, md, mn,
                  _ffi.ptr(node_ptr), m, _ffi.ptr(idx), _ffi.ptr(recv), _ffi.ptr(send), _ffi.ptr(dist), _ffi.stream())
        indices = RaggedTensor(idx, edge_splits)
        from ..ragged import IndexPlan
        indices.attach_plan(node_coordinates, IndexPlan.from_prepared(indices, node_coordinates, cols, node_ptr))
        return indices, RaggedTensor(dist, edge_splits)


class SetAngle:
    """Angle triples ``(i, j, k)``, edge pairs ``(n, m)`` and angle values of a ragged batch of edge lists, built on the
    device (``mp_angle_list_*``).  Keywords and defaults of the reference's ``SetAngle``
    (kgcnn/graph/preprocessor.py:337-342).  The order is by ``n``, then ``m`` ascending - what ``check_sorted=True``
    yields, so ``check_sorted`` changes nothing here.  ``allow_self_edges=True`` is not implemented."""

    def __init__(self, *, range_indices: str = "range_indices", node_coordinates: str = "node_coordinates",
                 angle_indices: str = "angle_indices", angle_indices_nodes: str = "angle_indices_nodes",
                 angle_attributes: str = "angle_attributes", allow_multi_edges: bool = False,
                 allow_self_edges: bool = False, allow_reverse_edges: bool = False, edge_pairing: str = "kj",
                 check_sorted: bool = True, compute_angles: bool = True, name="set_angle", **kwargs):
        if allow_self_edges:
            raise NotImplementedError("on-GPU SetAngle does not pair an edge with itself (allow_self_edges=True)")
        if "k" not in edge_pairing:
            raise ValueError("Edge pairing must have index 'k'.")
        if "i" not in edge_pairing and "j" not in edge_pairing:
            raise ValueError("Edge pairing must have at least one fix index 'i' or 'j'.")
        self.name = name
        self._config_kwargs = {"node_coordinates": node_coordinates, "range_indices": range_indices,
                               "angle_indices": angle_indices, "angle_indices_nodes": angle_indices_nodes,
                               "angle_attributes": angle_attributes, "allow_multi_edges": allow_multi_edges,
                               "compute_angles": compute_angles, "allow_self_edges": allow_self_edges,
                               "edge_pairing": edge_pairing, "allow_reverse_edges": allow_reverse_edges,
                               "check_sorted": check_sorted}
        self.allow_multi_edges, self.allow_reverse_edges = bool(allow_multi_edges), bool(allow_reverse_edges)
        self.compute_angles = bool(compute_angles)
        self.pos_k = 0 if edge_pairing[0] == "k" else 1       # kgcnn/graph/adj.py:335-337
        self.pos_fix = 1 - self.pos_k
        self.pos_ij = 0 if "i" in edge_pairing else 1

    def get_config(self):
        return {"name": self.name, **self._config_kwargs}

    @property
    def produces(self):
        """Property names this preprocessor adds when used on a dict of packed tensors (MD driver)."""
        names = (self._config_kwargs["angle_indices"], self._config_kwargs["angle_indices_nodes"])
        return names + ((self._config_kwargs["angle_attributes"],) if self.compute_angles else ())

    def __call__(self, range_indices, node_coordinates=None):
        if isinstance(range_indices, dict):  # dict of packed device tensors -> dict of the new properties
            out = self._run(range_indices[self._config_kwargs["range_indices"]],
                            range_indices[self._config_kwargs["node_coordinates"]])
            return {name: t for name, t in zip(self.produces, out)}
        return self._run(range_indices, node_coordinates)

    def _count(self, range_indices, eplan):
        """Pass 1: ``(off (M+1) int64, angle_splits (G+1) int64, A)`` of the edge list with index plan ``eplan``."""
        m, g, dev = eplan.M, eplan.G, eplan.cols.device
        off = torch.zeros(m + 1, dtype=torch.int64, device=dev)
        angle_splits = torch.zeros(g + 1, dtype=torch.int64, device=dev)
        if m == 0 or g == 0:
            return off, angle_splits, 0
        ptr, perm, _ = eplan.csr(self.pos_fix)
        nbytes = _ffi.workspace_bytes("mp_angle_list_workspace_bytes", m)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        _ffi.call("mp_angle_list_count_i32", _ffi.ptr(eplan.cols), m, eplan.N, _ffi.ptr(ptr), _ffi.ptr(perm),
                  _ffi.ptr(range_indices.row_splits), g, self.pos_fix, self.pos_ij, int(self.allow_multi_edges),
                  int(self.allow_reverse_edges), _ffi.ptr(off), _ffi.ptr(angle_splits), _ffi.ptr(ws), nbytes,
                  _ffi.stream())
        return off, angle_splits, int(off[-1].item())  # data-dependent output size: one host read, as in SetRange

    def _fill(self, range_indices, node_coordinates, eplan, off, a):
        """Pass 2: ``(triples (A,3), pairs (A,2), triple columns (3,A), pair columns (2,A), theta (A,1) or None,
        triple CSR (N+1) or None, pair CSR (M+1))`` for the ``off`` and ``A`` of :meth:`_count`."""
        m, n, dev = eplan.M, eplan.N, eplan.cols.device
        xyz = node_coordinates.values.contiguous()
        ptr, perm, _ = eplan.csr(self.pos_fix)
        sorted0 = eplan.is_sorted(0)
        triples = torch.empty((a, 3), dtype=torch.int64, device=dev)
        pairs = torch.empty((a, 2), dtype=torch.int64, device=dev)
        tcols = torch.empty((3, max(a, 1)), dtype=torch.int32, device=dev)
        pcols = torch.empty((2, max(a, 1)), dtype=torch.int32, device=dev)
        theta = torch.empty((a, 1), dtype=torch.float32, device=dev) if self.compute_angles else None
        tptr = torch.zeros(n + 1, dtype=torch.int32, device=dev) if sorted0 else None
        pptr = torch.zeros(m + 1, dtype=torch.int32, device=dev)
        eptr0 = eplan.csr(0)[0] if sorted0 else None
        _ffi.call("mp_angle_list_fill_f32", _ffi.ptr(eplan.cols), m, n, _ffi.ptr(ptr), _ffi.ptr(perm),
                  _ffi.ptr(node_coordinates.row_splits), _ffi.ptr(range_indices.row_splits), eplan.G, self.pos_fix,
                  self.pos_ij, self.pos_k, int(self.allow_multi_edges), int(self.allow_reverse_edges), _ffi.ptr(off), a,
                  _ffi.ptr(xyz), _ffi.ptr(triples), _ffi.ptr(pairs), _ffi.ptr(tcols), _ffi.ptr(pcols), _ffi.ptr(theta),
                  _ffi.ptr(eptr0), _ffi.ptr(tptr), _ffi.ptr(pptr), _ffi.stream())
        return triples, pairs, tcols, pcols, theta, tptr, pptr

    def _run(self, range_indices: RaggedTensor, node_coordinates: RaggedTensor):
        """``range_indices``: ragged ``(batch, [M], 2)`` int64; ``node_coordinates``: ragged ``(batch, [N], 3)`` float32.
        Returns ``(angle_indices, angle_indices_nodes, angle_attributes)``: ragged ``(batch, [A], 2)`` int64 edge pairs,
        ``(batch, [A], 3)`` int64 node triples and ``(batch, [A], 1)`` float32 angles (``None`` without
        ``compute_angles``).  Both index tensors carry a ready index plan: the triples against the coordinates'
        partition, the pairs against ``range_indices``' partition."""
        from ..ragged import IndexPlan
        _ffi.require_device(node_coordinates.values, range_indices.values, range_indices.row_splits,
                            node_coordinates.row_splits)
        if self.compute_angles and node_coordinates.values.dtype != torch.float32:
            raise TypeError("SetAngle expects float32 coordinates, got %s" % node_coordinates.values.dtype)
        eplan = range_indices.index_plan(node_coordinates)
        if eplan.K != 2:
            raise ValueError("SetAngle expects range indices of shape (batch, [M], 2)")
        off, angle_splits, a = self._count(range_indices, eplan)
        triples, pairs, tcols, pcols, theta, tptr, pptr = self._fill(range_indices, node_coordinates, eplan, off, a)
        angle_nodes = RaggedTensor(triples, angle_splits)
        angle_edges = RaggedTensor(pairs, angle_splits)
        # column 0 of the triples is the receiver column of the edge list, edge by edge: sorted where that one is;
        # column 0 of the pairs is the edge index itself: always sorted.  Column 1 is not claimed.
        oob = eplan.flags_host() & _ffi.MP_FLAG_OOB
        tflags = oob | _ffi.MP_FLAG_UNSORTED_COL1 | (0 if eplan.is_sorted(0) else _ffi.MP_FLAG_UNSORTED_COL0)
        angle_nodes.attach_plan(node_coordinates,
                                IndexPlan.from_prepared(angle_nodes, node_coordinates, tcols, tptr, flags=tflags))
        angle_edges.attach_plan(range_indices, IndexPlan.from_prepared(angle_edges, range_indices, pcols, pptr,
                                                                       flags=oob | _ffi.MP_FLAG_UNSORTED_COL1))
        return angle_edges, angle_nodes, (RaggedTensor(theta, angle_splits) if self.compute_angles else None)


class SetRangePeriodic:
    """Range connections of a ragged batch of periodic structures, built on the device (``mp_radius_graph_periodic_*``,
    csrc/mp_lattice.hip).  Keywords and defaults of the reference's ``SetRangePeriodic``
    (kgcnn/graph/preprocessor.py:393-411).

    Rule (``range_neighbour_lattice``, kgcnn/graph/geom.py:172-368, ``exclusive=True``, ``self_loops=False``): receiver
    ``i`` is connected to every sender ``j`` in image ``n`` with ``|x_j + n L - x_i| <= max_distance``; only ``(j = i,
    n = 0)`` is left out, so an atom's own images are neighbours.  Per receiver the neighbours come in ascending
    distance, cut after ``max_neighbours``; receivers in node order.  The lattice vectors are the rows of ``L``.

    Differences to the reference, both inside what it leaves undefined: the comparison is ``d <= max_distance`` on the
    float32 distance (the reference adds ``1e-8`` in float64, which is below float32 resolution at these magnitudes), and
    the order inside a tie - the reference's unstable ``argsort`` - is (float32 distance, sender id, image
    lexicographic).  Atoms need not be wrapped into the cell.

    Limits: ``MP_PERIODIC_MAX_HITS`` neighbours inside the cutoff per receiver (before the ``max_neighbours`` cut),
    ``MP_PERIODIC_MAX_CANDIDATES`` image-box candidates per receiver, image indices within ``+-MP_PERIODIC_MAX_IMAGE``,
    a non-singular lattice.  Exceeding one raises ``ValueError``; nothing is cut silently.

    ``self_loops=True``, ``exclusive=False``, ``do_invert_distance=True`` and ``max_distance=None`` are not implemented.
    """

    def __init__(self, *, range_indices: str = "range_indices", node_coordinates: str = "node_coordinates",
                 graph_lattice: str = "graph_lattice", range_image: str = "range_image",
                 range_attributes: str = "range_attributes", max_distance: float = 4.0, max_neighbours: int = None,
                 exclusive: bool = True, do_invert_distance: bool = False, self_loops: bool = False,
                 overwrite: bool = True, name="set_range_periodic", **kwargs):
        if self_loops or not exclusive or do_invert_distance or max_distance is None:
            raise NotImplementedError("on-GPU SetRangePeriodic covers: exclusive, no self loops, plain distances, a "
                                      "finite max_distance")
        self.name = name
        self._config_kwargs = {"node_coordinates": node_coordinates, "range_indices": range_indices,
                               "graph_lattice": graph_lattice, "range_image": range_image,
                               "range_attributes": range_attributes, "max_distance": max_distance,
                               "max_neighbours": max_neighbours, "exclusive": exclusive,
                               "do_invert_distance": do_invert_distance, "self_loops": self_loops,
                               "overwrite": overwrite}
        self.max_distance = float(max_distance)
        self.max_neighbours = max_neighbours
        self.overwrite = bool(overwrite)

    def get_config(self):
        return {"name": self.name, **self._config_kwargs}

    @property
    def produces(self):
        """Property names this preprocessor adds when used on a dict of packed tensors (MD driver)."""
        return (self._config_kwargs["range_indices"], self._config_kwargs["range_image"],
                self._config_kwargs["range_attributes"])

    def __call__(self, node_coordinates, graph_lattice=None, range_indices=None, range_image=None):
        """``(node_coordinates, graph_lattice)`` -> ``(range_indices, range_image, range_attributes)``, or a dict of packed
        device tensors -> dict of the three properties.  With ``overwrite=False`` and both ``range_indices`` and
        ``range_image`` given (as arguments, or present in the dict) only the distances are recomputed."""
        if isinstance(node_coordinates, dict):
            t, cfg = node_coordinates, self._config_kwargs
            out = self._dispatch(t[cfg["node_coordinates"]], t[cfg["graph_lattice"]], t.get(cfg["range_indices"]),
                                 t.get(cfg["range_image"]))
            return {name: v for name, v in zip(self.produces, out)}
        return self._dispatch(node_coordinates, graph_lattice, range_indices, range_image)

    def _dispatch(self, xyz, lattice, indices, image):
        if lattice is None:
            raise ValueError("SetRangePeriodic needs the lattice matrices (batch, 3, 3)")
        if not self.overwrite and indices is not None and image is not None:
            return indices, image, self._distances(xyz, lattice, indices, image)
        return self._run(xyz, lattice)

    @staticmethod
    def _check(node_coordinates, graph_lattice):
        xyz = node_coordinates.values.contiguous()
        _ffi.require_device(xyz, node_coordinates.row_splits, graph_lattice)
        g = node_coordinates.nrows()
        if xyz.dtype != torch.float32 or graph_lattice.dtype != torch.float32:
            raise TypeError("SetRangePeriodic expects float32 coordinates and lattice")
        if tuple(graph_lattice.shape) != (g, 3, 3):
            raise ValueError("graph_lattice must have shape (%d, 3, 3), got %s" % (g, tuple(graph_lattice.shape)))
        return xyz, graph_lattice.contiguous(), g

    @staticmethod
    def _distances(node_coordinates, graph_lattice, range_indices, range_image):
        """``range_attributes`` of a given edge list: gather, shift, norm - the layers the crystal models run."""
        from ..layers.geom import NodeDistanceEuclidean, NodePosition, ShiftPeriodicLattice
        with torch.no_grad():
            pos1, pos2 = NodePosition()([node_coordinates, range_indices])
            pos2 = ShiftPeriodicLattice()([pos2, range_image, graph_lattice])
            return NodeDistanceEuclidean()([pos1, pos2])

    def _run(self, node_coordinates: RaggedTensor, graph_lattice):
        """``node_coordinates``: ragged ``(batch, [N], 3)`` float32; ``graph_lattice``: ``(batch, 3, 3)`` float32.
        Returns ragged ``(batch, [M], 2)`` int64 sample indices carrying a ready index plan (column 0 sorted, column 1 not
        claimed), ragged ``(batch, [M], 3)`` int64 images and ragged ``(batch, [M], 1)`` float32 distances."""
        from ..ragged import IndexPlan
        xyz, lat, g = self._check(node_coordinates, graph_lattice)
        n, dev = int(xyz.shape[0]), xyz.device
        mn = -1 if self.max_neighbours is None else int(min(self.max_neighbours, 2 ** 30))
        nbytes = _ffi.workspace_bytes("mp_radius_graph_periodic_workspace_bytes", n)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        head = torch.empty(n + 2, dtype=torch.int32, device=dev)   # node_ptr (N+1), then the flag word
        node_ptr, flags = head[:n + 1], head[n + 1:]
        edge_splits = torch.empty(g + 1, dtype=torch.int64, device=dev)
        _ffi.call("mp_radius_graph_periodic_count_f32", _ffi.ptr(xyz), _ffi.ptr(node_coordinates.row_splits),
                  _ffi.ptr(lat), g, n, self.max_distance, mn, _ffi.ptr(node_ptr), _ffi.ptr(edge_splits),
                  _ffi.ptr(flags), _ffi.ptr(ws), nbytes, _ffi.stream())
        m, bits = (int(v) for v in head[n:].tolist())   # the one host read: output size and limit flags together
        if bits:
            raise ValueError("SetRangePeriodic(max_distance=%g): %s" % (self.max_distance, "; ".join(
                text for bit, text in (
                    (_ffi.MP_PERIODIC_FLAG_CAPACITY, "a receiver has more than %d neighbours inside the cutoff or more "
                     "than %d image candidates" % (_ffi.MP_PERIODIC_MAX_HITS, _ffi.MP_PERIODIC_MAX_CANDIDATES)),
                    (_ffi.MP_PERIODIC_FLAG_IMAGE_RANGE, "an image index exceeds +-%d" % _ffi.MP_PERIODIC_MAX_IMAGE),
                    (_ffi.MP_PERIODIC_FLAG_SINGULAR, "a lattice is singular (cell volume ~ 0)")) if bits & bit)))
        idx = torch.empty((m, 2), dtype=torch.int64, device=dev)
        image = torch.empty((m, 3), dtype=torch.int64, device=dev)
        cols = torch.empty((2, max(m, 1)), dtype=torch.int32, device=dev)
        dist = torch.empty((m, 1), dtype=torch.float32, device=dev)
        _ffi.call("mp_radius_graph_periodic_fill_f32", _ffi.ptr(xyz), _ffi.ptr(node_coordinates.row_splits),
                  _ffi.ptr(lat), g, n, self.max_distance, mn, _ffi.ptr(node_ptr), m, _ffi.ptr(idx), _ffi.ptr(image),
                  _ffi.ptr(cols[0]), _ffi.ptr(cols[1]), _ffi.ptr(dist), _ffi.stream())
        indices = RaggedTensor(idx, edge_splits)
        indices.attach_plan(node_coordinates, IndexPlan.from_prepared(indices, node_coordinates, cols, node_ptr))
        return indices, RaggedTensor(image, edge_splits), RaggedTensor(dist, edge_splits)
