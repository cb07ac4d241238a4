"""Restatement of the periodic-cell pieces for the tests (torch on the CPU / NumPy, float32 or float64): the lattice shift
of ``ShiftPeriodicLattice`` (kgcnn/layers/geom.py:119-120), the neighbour rule of ``range_neighbour_lattice``
(kgcnn/graph/geom.py:172-368, ``exclusive=True``, ``self_loops=False``) by brute-force enumeration, and the energies of
the two crystal models.

TEST INFRASTRUCTURE, NOT PRODUCT CODE.  The energies are ``oracle/torch_force_oracle.py``'s ``schnet_energy`` /
``painn_energy`` with that module's ``_distance`` - the one function both take all their geometry from - replaced for
the duration of the call (pytest's ``monkeypatch``) by ``x_i - (x_j + n L)``.  tests/test_periodic_api.py pins this file
on the CPU: its neighbour sets equal the golden sets of the reference, and its energies obey the super-cell and the
lattice-translation identities in float64.
"""
import itertools

import numpy as np
import torch

from oracle import torch_force_oracle as tfo


def lattice_shift_np(pos, image, lattice_of_edge, dtype=np.float32):
    """``pos + ((n0 a0 + n1 a1) + n2 a2)`` per edge in ``dtype``, the reference's ``reduce_sum`` order; NumPy does not
    contract a product into the following sum, so in float32 this is what the engine computes bit for bit.
    ``lattice_of_edge``: ``(M, 3, 3)``, lattice vectors in rows."""
    p, lat = np.asarray(pos, dtype), np.asarray(lattice_of_edge, dtype)
    n = np.asarray(image).astype(dtype)
    prod = lat * n[:, :, None]                       # (M, 3 rows, 3 components)
    return p + ((prod[:, 0] + prod[:, 1]) + prod[:, 2])


def lattice_of_edge(lattice, edge_splits):
    es = np.asarray(edge_splits, np.int64)
    return np.repeat(np.asarray(lattice), es[1:] - es[:-1], axis=0)


def edge_distances_np(xyz, idx, image, lattice, dtype=np.float32):
    """Distances of one structure's edges the way the engine's neighbour search and its layers compute them:
    ``|(x_j + shift) - x_i|``, ``sqrt((e0^2 + e1^2) + e2^2)`` in ``dtype``."""
    x = np.asarray(xyz, dtype)
    lat = np.broadcast_to(np.asarray(lattice, dtype), (len(idx), 3, 3))
    e = lattice_shift_np(x[idx[:, 1]], image, lat, dtype) - x[idx[:, 0]]
    sq = e * e
    return np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2])


def neighbours(xyz, lattice, max_distance, max_neighbours=None, dtype=np.float64):
    """Brute force over a box of images that is a superset of the cutoff sphere (perpendicular heights of the cell plus
    the spread of the atoms in fractional coordinates, plus one).  Returns ``(indices (M, 2), images (M, 3), dist (M,))``
    in the engine's order: receivers ascending; per receiver by (distance in ``dtype``, sender, image lexicographic),
    cut after ``max_neighbours``."""
    x64, l64 = np.asarray(xyz, np.float64), np.asarray(lattice, np.float64)
    n = len(x64)
    vol = abs(np.dot(l64[0], np.cross(l64[1], l64[2])))
    heights = [vol / np.linalg.norm(np.cross(l64[(k + 1) % 3], l64[(k + 2) % 3])) for k in range(3)]
    frac = x64 @ np.linalg.inv(l64)
    spread = (frac.max(axis=0) - frac.min(axis=0)) if n else np.zeros(3)
    reach = [int(np.ceil(max_distance / heights[k] + spread[k])) + 1 for k in range(3)]
    images = np.array(list(itertools.product(*[range(-r, r + 1) for r in reach])), dtype=np.int64)
    idx_out, img_out, d_out = [], [], []
    for i in range(n):
        rows = []
        for j in range(n):
            pairs = np.stack([np.full(len(images), i), np.full(len(images), j)], axis=1)
            d = edge_distances_np(xyz, pairs, images, lattice, dtype)
            keep = d <= dtype(max_distance)
            if i == j:
                keep &= np.any(images != 0, axis=1)
            for m in np.nonzero(keep)[0]:
                rows.append((d[m], j) + tuple(int(v) for v in images[m]))
        rows.sort()
        if max_neighbours is not None:
            rows = rows[:max_neighbours]
        for r in rows:
            idx_out.append((i, r[1]))
            img_out.append(r[2:])
            d_out.append(r[0])
    return (np.asarray(idx_out, np.int64).reshape(-1, 2), np.asarray(img_out, np.int64).reshape(-1, 3),
            np.asarray(d_out, dtype).reshape(-1))


def edge_set(indices, images):
    """The edge list as a set of ``(i, j, n0, n1, n2)`` (the order inside ties is not part of the rule)."""
    return set(tuple(int(v) for v in np.concatenate([a, b])) for a, b in zip(indices, images))


def batch(structures, max_distance, max_neighbours=None, numbers=None, dtype=np.float64):
    """Concatenate ``[(xyz, lattice), ...]`` into one ragged batch with the restatement's neighbour lists."""
    xs, idxs, imgs, ds = [], [], [], []
    for xyz, lat in structures:
        i, m, d = neighbours(xyz, lat, max_distance, max_neighbours, dtype)
        xs.append(np.asarray(xyz, np.float32).reshape(-1, 3)), idxs.append(i), imgs.append(m), ds.append(d)
    ns = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    es = np.concatenate([[0], np.cumsum([len(i) for i in idxs])]).astype(np.int64)
    b = {"node_coordinates": np.concatenate(xs, axis=0), "node_splits": ns, "edge_splits": es,
         "edge_indices": np.concatenate(idxs, axis=0), "edge_image": np.concatenate(imgs, axis=0),
         "edge_distance": np.concatenate(ds), "graph_lattice": np.stack([np.asarray(l, np.float32) for _, l in structures])}
    if numbers is None:
        rng = np.random.default_rng(int(ns[-1]))
        numbers = rng.choice(np.array([1, 6, 7, 8], dtype=np.int64), size=int(ns[-1]))
    b["node_number"] = np.asarray(numbers, np.int64)
    return b


def _periodic_distance(image, lattice, edge_splits, dtype):
    shift_rows = torch.from_numpy(lattice_of_edge(lattice, edge_splits)).to(dtype)       # (M, 3, 3)
    n = torch.from_numpy(np.asarray(image, np.int64)).to(dtype)

    def distance(xyz, sh):
        prod = shift_rows * n.unsqueeze(-1)
        shift = (prod[:, 0] + prod[:, 1]) + prod[:, 2]
        diff = xyz.index_select(0, sh[:, 0]) - (xyz.index_select(0, sh[:, 1]) + shift)
        return diff, torch.sqrt(torch.relu(diff.square().sum(-1, keepdim=True)))

    return distance


def crystal_energy(monkeypatch, kind, p, b, xyz=None, dtype=torch.float64, **kw):
    """Energy ``(G, states)`` of the crystal SchNet (``kind="schnet"``) or PaiNN (``"painn"``) on batch ``b`` with the
    weights ``p`` (a dict of torch tensors in ``dtype``, ``tfo.to_torch``); differentiable in ``xyz`` and ``p``."""
    x = torch.from_numpy(b["node_coordinates"]).to(dtype) if xyz is None else xyz
    fn = {"schnet": tfo.schnet_energy, "painn": tfo.painn_energy}[kind]
    with monkeypatch.context() as m:
        m.setattr(tfo, "_distance", _periodic_distance(b["edge_image"], b["graph_lattice"], b["edge_splits"], dtype))
        return fn(p, b["node_number"], x, b["edge_indices"], b["node_splits"], b["edge_splits"], **kw)


def crystal_energy_force(monkeypatch, kind, params, b, dtype=torch.float64, **kw):
    """Energies ``(G, 1)`` and physical forces ``(N, 3)`` as NumPy arrays."""
    p = tfo.to_torch(params, dtype)
    x = torch.from_numpy(b["node_coordinates"]).to(dtype).requires_grad_(True)
    e = crystal_energy(monkeypatch, kind, p, b, xyz=x, dtype=dtype, **kw)
    g, = torch.autograd.grad(e.sum(), x)
    return e.detach().numpy(), (-g).numpy()


def golden_cases(golden_dir):
    """``{name: dict(xyz, lattice, cutoff, maxn, indices, images, dist)}`` of tests/golden/periodic_cases.npz."""
    import os
    z = np.load(os.path.join(golden_dir, "periodic_cases.npz"))
    out = {}
    for name in [str(s) for s in z["names"]]:
        maxn = int(z["maxn_" + name])
        out[name] = {"xyz": z["xyz_" + name], "lattice": z["lattice_" + name], "cutoff": float(z["cutoff_" + name]),
                     "maxn": None if maxn < 0 else maxn, "indices": z["indices_" + name],
                     "images": z["images_" + name], "dist": z["dist_" + name]}
    return out
