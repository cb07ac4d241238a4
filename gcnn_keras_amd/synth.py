"""Synthetic ragged batches shaped like the reference's benchmark datasets (host side, NumPy only).

The GPU box has neither the reference tree nor any dataset, so the inputs of every BASELINE.json
config are generated here from ``numpy.random.default_rng(seed)``.  The
edge rule restates ``kgcnn.graph.adj.define_adjacency_from_distance`` (kgcnn/graph/adj.py:537-593,
as called by ``SetRange``, kgcnn/graph/preprocessor.py:288-314): connect ``i -> j`` when
``dist < max_distance`` AND ``j`` is among the ``max_neighbours + 1`` nearest entries of row ``i``
(exclusive mode), no self loops, indices in row-major ``(i, j)`` order - hence sorted by receiver.
tests/test_synth.py checks it against edge lists produced in the build container by the reference's
own function (tests/golden/radius_graph_cases.npz).
"""
import numpy as np


def distance_matrix(xyz):
    """kgcnn/graph/adj.py:466-483: ``sqrt(sum((b - a)^2))`` in the coordinate dtype."""
    xyz = np.asarray(xyz)
    c = xyz[:, None, :] - xyz[None, :, :]
    return np.sqrt(np.sum(np.square(c), axis=-1))


def radius_graph(xyz, max_distance=4.0, max_neighbours=30):
    """Edge list ``(m, 2)`` int64 of one molecule by the reference rule (exclusive, no self loops)."""
    dist = distance_matrix(xyz)
    n = dist.shape[-1]
    adj = np.ones_like(dist, dtype=bool)
    if max_distance is not None:
        adj &= dist < max_distance
    if max_neighbours is not None:
        k = min(int(max_neighbours), n)
        order = np.argsort(dist, axis=-1)[..., :k + 1]
        temp = np.zeros_like(dist, dtype=bool)
        np.put_along_axis(temp, order, True, axis=-1)
        adj &= temp
    adj[np.arange(n), np.arange(n)] = False
    ii, jj = np.nonzero(adj)  # row-major order == graph_indices[graph_adjacency]
    return np.stack([ii, jj], axis=-1).astype(np.int64)


def _splits(lengths):
    return np.concatenate([np.zeros(1, np.int64), np.cumsum(np.asarray(lengths, dtype=np.int64))])


def qm9_like_nodes(num_graphs=128, seed=1234, sigma=1.6):
    """Node side of :func:`qm9_like_batch` alone (same draws): numbers, coordinates and node row_splits.  The edge lists
    of large batches (BASELINE config 4: 100 000 molecules) are then built on the GPU by the engine's ``SetRange``
    (gcnn_keras_amd/graph/preprocessor.py), which applies the same rule as :func:`radius_graph`."""
    rng = np.random.default_rng(seed)
    rng_z = np.random.default_rng(seed + 1)
    z_vals = np.array([1, 6, 7, 8, 9], dtype=np.float32)
    z_p = np.array([.51, .35, .06, .07, .01])
    zs, xs, n_len = [], [], []
    for _ in range(num_graphs):
        n = int(np.clip(np.rint(rng.normal(18.0, 4.5)), 3, 29))
        xs.append(rng.normal(0.0, sigma, size=(n, 3)).astype(np.float32))
        zs.append(rng_z.choice(z_vals, size=n, p=z_p).astype(np.float32))
        n_len.append(n)
    return {"node_number": np.concatenate(zs), "node_coordinates": np.concatenate(xs, axis=0),
            "node_splits": _splits(n_len)}


def qm9_like_batch(num_graphs=128, seed=1234, sigma=1.6, max_distance=4.0, max_neighbours=30):
    """BASELINE config 2: QM9-shaped molecules.

    ``n_g = clip(round(N(18, 4.5^2)), 3, 29)``; ``Z`` from {1,6,7,8,9} w.p. {.51,.35,.06,.07,.01}
    as float32 (kgcnn/literature/Schnet.py:26 declares float node numbers); ``xyz ~ N(0, sigma^2 I)``;
    draw order per graph: n_g, then xyz (as in BASELINE.md's calibration: seed 1234 -> N=2301, M=26190);
    Z comes from a second stream (seed + 1).  Returns a dict of flat values + int64 row_splits.
    """
    out = qm9_like_nodes(num_graphs, seed, sigma)
    ns = out["node_splits"]
    es = [radius_graph(out["node_coordinates"][ns[g]:ns[g + 1]], max_distance=max_distance,
                       max_neighbours=max_neighbours) for g in range(num_graphs)]
    out["edge_indices"] = np.concatenate(es, axis=0).reshape(-1, 2).astype(np.int64)
    out["edge_splits"] = _splits([len(e) for e in es])
    return out


ASPIRIN_Z = np.array([6] * 9 + [1] * 8 + [8] * 4, dtype=np.float32)  # C9 H8 O4


def md17_like_batch(num_graphs=64, seed=2345, sigma=1.7, max_distance=5.0, max_neighbours=10000):
    """BASELINE config 3: 21-atom aspirin-composition molecules, cutoff 5 A, unlimited neighbours
    (training/hyper/hyper_md17.py:149)."""
    rng = np.random.default_rng(seed)
    zs, xs, es, n_len, e_len = [], [], [], [], []
    for _ in range(num_graphs):
        xyz = rng.normal(0.0, sigma, size=(21, 3)).astype(np.float32)
        ei = radius_graph(xyz, max_distance=max_distance, max_neighbours=max_neighbours)
        zs.append(ASPIRIN_Z.copy()); xs.append(xyz); es.append(ei); n_len.append(21); e_len.append(len(ei))
    return {
        "node_number": np.concatenate(zs), "node_coordinates": np.concatenate(xs, axis=0),
        "edge_indices": np.concatenate(es, axis=0).reshape(-1, 2).astype(np.int64),
        "node_splits": _splits(n_len), "edge_splits": _splits(e_len),
    }


def rescale_edge_weights_degree_sym(edge_indices, edge_weights):
    """``d_ii^-0.5 e_ij d_jj^-0.5`` with degree = occurrence count of the index in column 0 / 1
    (restates kgcnn/graph/adj.py:51-78)."""
    if len(edge_indices) == 0:
        return np.array([])
    row_val, row_cnt = np.unique(edge_indices[:, 0], return_counts=True)
    col_val, col_cnt = np.unique(edge_indices[:, 1], return_counts=True)
    d_row = np.zeros(len(edge_weights), dtype=edge_weights.dtype)
    d_col = np.zeros(len(edge_weights), dtype=edge_weights.dtype)
    d_row[row_val] = row_cnt
    d_col[col_val] = col_cnt
    with np.errstate(divide="ignore", invalid="ignore"):
        d_ii = np.nan_to_num(np.power(d_row, -0.5).flatten(), nan=0.0, posinf=0.0, neginf=0.0)
        d_jj = np.nan_to_num(np.power(d_col, -0.5).flatten(), nan=0.0, posinf=0.0, neginf=0.0)
    return d_ii[edge_indices[:, 0]][:, None] * edge_weights * d_jj[edge_indices[:, 1]][:, None]


def cora_like_graph(num_nodes=2708, attach=2, num_features=1433, density=0.0127, seed=4567, drop_pairs=134):
    """BASELINE config 5: one Cora-shaped graph.

    Barabasi-Albert preferential attachment (own implementation, ``attach`` edges per new node),
    ``drop_pairs`` undirected pairs removed uniformly -> both directions, sorted by (i, j), plus self
    loops, symmetric degree normalisation of unit weights (pipeline of training/hyper/hyper_cora.py:51-53),
    Bernoulli(density) features.
    """
    rng = np.random.default_rng(seed)
    targets = list(range(attach))
    repeated = []
    pairs = set()
    for src in range(attach, num_nodes):
        for t in set(targets):
            pairs.add((min(src, t), max(src, t)))
        repeated.extend(targets)
        repeated.extend([src] * attach)
        targets = []
        while len(targets) < attach:
            c = repeated[int(rng.integers(len(repeated)))]
            if c not in targets:
                targets.append(c)
    pairs = np.array(sorted(pairs), dtype=np.int64)
    if drop_pairs > 0:
        keep = np.ones(len(pairs), dtype=bool)
        keep[rng.choice(len(pairs), size=drop_pairs, replace=False)] = False
        pairs = pairs[keep]
    directed = np.concatenate([pairs, pairs[:, ::-1]], axis=0)
    loops = np.stack([np.arange(num_nodes), np.arange(num_nodes)], axis=-1)
    ei = np.concatenate([directed, loops], axis=0)
    order = np.lexsort((ei[:, 1], ei[:, 0]))
    ei = ei[order].astype(np.int64)
    w = rescale_edge_weights_degree_sym(ei, np.ones((len(ei), 1), dtype=np.float32)).astype(np.float32)
    x = (rng.random((num_nodes, num_features)) < density).astype(np.float32)
    return {
        "node_attributes": x, "edge_weights": w, "edge_indices": ei,
        "node_splits": _splits([num_nodes]), "edge_splits": _splits([len(ei)]),
    }


def toy_batch():
    """BASELINE config 1: the 3-graph README batch (README.md:84), F=3, values arange(18)/8."""
    idx = [[[0, 1], [1, 0]], [[0, 1], [1, 2], [2, 0]], [[0, 0]]]
    ei = np.concatenate([np.asarray(x, dtype=np.int64) for x in idx], axis=0)
    return {
        "node_attributes": (np.arange(18, dtype=np.float32).reshape(6, 3) / np.float32(8)),
        "edge_indices": ei,
        "node_splits": _splits([2, 3, 1]), "edge_splits": _splits([2, 3, 1]),
    }


def glorot_uniform(rng, fan_in, fan_out, shape=None):
    """Keras ``glorot_uniform``: U(-l, l), l = sqrt(6 / (fan_in + fan_out))."""
    limit = np.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-limit, limit, size=shape or (fan_in, fan_out)).astype(np.float32)


def schnet_params(seed=7, depth=3, units=128, emb_in=95, emb_out=64, bins=20, last_units=(128, 64),
                  out_units=(64, 1), random_bias=False):
    """Random-init SchNet weights in constructor order (shapes: SURVEY.md section 8a 'Parameter shapes';
    kgcnn/literature/Schnet.py:24-43, kgcnn/layers/conv/schnet_conv.py:50-51,136-139).
    Keras zero-initialises biases; ``random_bias=True`` draws small biases so parity tests exercise them."""
    rng = np.random.default_rng(seed)

    def bias(n):
        return (rng.uniform(-0.1, 0.1, size=n).astype(np.float32) if random_bias else np.zeros(n, np.float32))

    p = {"embedding": rng.uniform(-0.05, 0.05, size=(emb_in, emb_out)).astype(np.float32),
         "dense0/kernel": glorot_uniform(rng, emb_out, units), "dense0/bias": bias(units)}
    for i in range(depth):
        pre = "interaction%d/" % i
        p[pre + "cfconv/dense1/kernel"] = glorot_uniform(rng, bins, units)
        p[pre + "cfconv/dense1/bias"] = bias(units)
        p[pre + "cfconv/dense2/kernel"] = glorot_uniform(rng, units, units)
        p[pre + "cfconv/dense2/bias"] = bias(units)
        p[pre + "dense1/kernel"] = glorot_uniform(rng, units, units)
        p[pre + "dense2/kernel"] = glorot_uniform(rng, units, units)
        p[pre + "dense2/bias"] = bias(units)
        p[pre + "dense3/kernel"] = glorot_uniform(rng, units, units)
        p[pre + "dense3/bias"] = bias(units)
    fan = units
    for k, u in enumerate(last_units):
        p["last_mlp/%d/kernel" % k] = glorot_uniform(rng, fan, u)
        p["last_mlp/%d/bias" % k] = bias(u)
        fan = u
    for k, u in enumerate(out_units):
        p["output_mlp/%d/kernel" % k] = glorot_uniform(rng, fan, u)
        p["output_mlp/%d/bias" % k] = bias(u)
        fan = u
    return p


def painn_params(seed=8, depth=3, units=128, emb_in=95, num_radial=20, out_units=(128, 1), random_bias=False):
    """Random-init PaiNN weights (kgcnn/layers/conv/painn_conv.py:54-56,167-170; kgcnn/literature/PAiNN.py:24-42)."""
    rng = np.random.default_rng(seed)

    def bias(n):
        return (rng.uniform(-0.1, 0.1, size=n).astype(np.float32) if random_bias else np.zeros(n, np.float32))

    p = {"embedding": rng.uniform(-0.05, 0.05, size=(emb_in, units)).astype(np.float32),
         "bessel/frequencies": (np.pi * np.arange(1, num_radial + 1, dtype=np.float32))}
    for i in range(depth):
        c = "conv%d/" % i
        p[c + "dense1/kernel"] = glorot_uniform(rng, units, units); p[c + "dense1/bias"] = bias(units)
        p[c + "phi/kernel"] = glorot_uniform(rng, units, 3 * units); p[c + "phi/bias"] = bias(3 * units)
        p[c + "w/kernel"] = glorot_uniform(rng, num_radial, 3 * units); p[c + "w/bias"] = bias(3 * units)
        u = "update%d/" % i
        p[u + "dense1/kernel"] = glorot_uniform(rng, 2 * units, units); p[u + "dense1/bias"] = bias(units)
        p[u + "lin_u/kernel"] = glorot_uniform(rng, units, units)
        p[u + "lin_v/kernel"] = glorot_uniform(rng, units, units)
        p[u + "a/kernel"] = glorot_uniform(rng, units, 3 * units); p[u + "a/bias"] = bias(3 * units)
    fan = units
    for k, uu in enumerate(out_units):
        p["output_mlp/%d/kernel" % k] = glorot_uniform(rng, fan, uu)
        p["output_mlp/%d/bias" % k] = bias(uu)
        fan = uu
    return p


def gcn_params(seed=9, depth=3, in_features=1433, units=64, out_units=(64, 32, 7), random_bias=False):
    """Random-init GCN weights (kgcnn/literature/GCN.py:95-97, kgcnn/layers/conv/gcn_conv.py:63-66)."""
    rng = np.random.default_rng(seed)

    def bias(n):
        return (rng.uniform(-0.1, 0.1, size=n).astype(np.float32) if random_bias else np.zeros(n, np.float32))

    p = {"dense0/kernel": glorot_uniform(rng, in_features, units), "dense0/bias": bias(units)}
    for i in range(depth):
        p["gcn%d/kernel" % i] = glorot_uniform(rng, units, units)
        p["gcn%d/bias" % i] = bias(units)
    fan = units
    for k, u in enumerate(out_units):
        p["output_mlp/%d/kernel" % k] = glorot_uniform(rng, fan, u)
        p["output_mlp/%d/bias" % k] = bias(u)
        fan = u
    return p


# ---------------------------------------------------------------------------------------------------------- HDNNP2nd
BOHR_PER_ANGSTROM = 1.8897261246257702
# Alanine dipeptide, C6 H12 N2 O2 (the fork's force_hdnnp2nd.py dataset "Alanindipeptide")
ALANINE_DIPEPTIDE_Z = np.array([1, 6, 1, 1, 6, 8, 7, 1, 6, 1, 6, 1, 1, 1, 6, 8, 7, 1, 6, 1, 1, 1], dtype=np.int64)

# The fork's symmetry-function and network table (force_hdnnp2nd.py:43-65): distances in Bohr.
HDNNP_FORK = {
    "cutoff_rad": 20.0, "rs": [0.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0], "eta": [0.03, 0.08, 0.16, 0.3, 0.5],
    "cutoff_ang": 12.0, "lamda": [-1.0, 1.0], "zeta": [1.0, 2.0, 4.0, 8.0, 16.0], "eta_ang": [0.03, 0.08, 0.16, 0.3, 0.5],
    "max_elements": 30, "elements": [1, 6, 7, 8], "hidden": [35, 35], "hidden_activation": ["tanh", "tanh"],
    "multiplicity": 2.0,
}


def hdnnp_model_kwargs(fork=HDNNP_FORK):
    """``make_model_behler`` keyword arguments of the fork's force_hdnnp2nd.py:139-174 (custom tanh as "tanh")."""
    return {
        "g2_kwargs": {"eta": list(fork["eta"]), "rs": list(fork["rs"]), "rc": fork["cutoff_rad"],
                      "elements": list(fork["elements"])},
        "g4_kwargs": {"eta": list(fork["eta_ang"]), "zeta": list(fork["zeta"]), "lamda": list(fork["lamda"]),
                      "rc": fork["cutoff_ang"], "elements": list(fork["elements"]), "multiplicity": fork["multiplicity"]},
        "normalize_kwargs": {},
        "mlp_kwargs": {"units": list(fork["hidden"]) + [1], "num_relations": fork["max_elements"],
                       "activation": list(fork["hidden_activation"]) + ["linear"]},
        "node_pooling_args": {"pooling_method": "sum"},
        "output_embedding": "graph", "output_to_tensor": True, "use_output_mlp": False,
    }


def angle_indices(idx, edge_pairing="kj"):
    """Angle triples ``(i, j, k)`` of one molecule's edge list: a NumPy restatement of kgcnn/graph/adj.py::
    get_angle_indices with SetAngle's defaults (no multi, self or reverse edges).  For edge ``n = (i, j)`` the partner
    edges ``m`` are those whose fixed end (``edge_pairing``: "kj" - column 1, "ik" - column 0) equals the edge's
    (column 1 for "kj", column 0 for "ik"); the triple is ``(i, j, idx[m, k-position])``; order: by n, then m."""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1, 2)
    if len(idx) == 0:
        return np.zeros((0, 3), np.int64)
    pos_k = 0 if edge_pairing[0] == "k" else 1
    pos_fix = 1 if edge_pairing[0] == "k" else 0
    pos_ij = 0 if "i" in edge_pairing else 1
    a, b = idx[:, None, :], idx[None, :, :]
    mask = b[..., pos_fix] == a[..., pos_ij]
    mask &= (b[..., 0] != a[..., 0]) | (b[..., 1] != a[..., 1])      # multi edges
    mask &= (b[..., 0] != a[..., 1]) | (b[..., 1] != a[..., 0])      # reverse edges
    np.fill_diagonal(mask, False)                                    # self
    n, m = np.nonzero(mask)
    return np.concatenate([idx[n], idx[m, pos_k][:, None]], axis=-1).astype(np.int64)


def hdnnp_batch(num_graphs=128, seed=3456, sigma=1.5, min_distance=0.9, z=ALANINE_DIPEPTIDE_Z, fork=HDNNP_FORK,
                edge_pairing="kj"):
    """Alanine-dipeptide-shaped molecules for HDNNP2nd: 22 atoms (H/C/N/O), coordinates ``N(0, sigma^2)`` in Angstrom
    redrawn per atom until every pair is at least ``min_distance`` apart, stored in Bohr.  Range indices by the fork's
    radius, ``cutoff_rad`` + 1 Angstrom in Bohr (all pairs within it, no neighbour limit); angle indices by
    :func:`angle_indices`."""
    rng = np.random.default_rng(seed)
    radius = fork["cutoff_rad"] + BOHR_PER_ANGSTROM
    zs, xs, es, ts = [], [], [], []
    for _ in range(num_graphs):
        xyz = np.zeros((len(z), 3))
        for a in range(len(z)):
            while True:
                p = rng.normal(0.0, sigma, size=3)
                if a == 0 or np.min(np.linalg.norm(xyz[:a] - p, axis=-1)) >= min_distance:
                    break
            xyz[a] = p
        xyz = (xyz * BOHR_PER_ANGSTROM).astype(np.float32)
        ei = radius_graph(xyz, max_distance=radius, max_neighbours=None)
        zs.append(np.asarray(z, np.int64)); xs.append(xyz); es.append(ei); ts.append(angle_indices(ei, edge_pairing))
    return {
        "node_number": np.concatenate(zs), "node_coordinates": np.concatenate(xs, axis=0),
        "edge_indices": np.concatenate(es, axis=0).reshape(-1, 2).astype(np.int64),
        "angle_indices": np.concatenate(ts, axis=0).reshape(-1, 3).astype(np.int64),
        "node_splits": _splits([len(x) for x in xs]), "edge_splits": _splits([len(e) for e in es]),
        "angle_splits": _splits([len(t) for t in ts]),
    }


def hdnnp_params(seed=10, fork=HDNNP_FORK, random_bias=True):
    """Random RelationalMLP weights of the fork's HDNNP2nd in ``model.weights`` order: per layer ``kernel``
    ``(max_elements, in, units)`` (Glorot per relation) and ``bias``; ``in`` = 140 radial + 500 angular functions."""
    rng = np.random.default_rng(seed)
    n_el = len(fork["elements"])
    fan = len(fork["rs"]) * len(fork["eta"]) * n_el + \
        len(fork["eta_ang"]) * len(fork["zeta"]) * len(fork["lamda"]) * (n_el * (n_el + 1) // 2)
    p = {}
    for k, u in enumerate(list(fork["hidden"]) + [1]):
        p["mlp/%d/kernel" % k] = glorot_uniform(rng, fan, u, shape=(fork["max_elements"], fan, u))
        p["mlp/%d/bias" % k] = (rng.uniform(-0.1, 0.1, size=u).astype(np.float32) if random_bias
                                else np.zeros(u, np.float32))
        fan = u
    return p


# ---------------------------------------------------------------------------------------------------------- HDNNP4th
# The fork's HDNNP4th table (force_hdnnp4th.py:41-71, charge_hdnnp4th.py): the HDNNP2nd symmetry functions, a [15] tanh
# charge network and the [35, 35] tanh local network.
HDNNP4TH_FORK = dict(HDNNP_FORK, charge_hidden=[15], charge_hidden_activation=["tanh"])
MIXED_SIZES = (1, 2, 3, 22, 128)   # the molecule sizes of hdnnp4th_batch(mixed=True); 128 = the charge solve's bound


def hdnnp4th_model_kwargs(fork=HDNNP4TH_FORK, output_embedding="charge+qm_energy"):
    """``HDNNP4th.make_model_behler`` keyword arguments of the fork's force_hdnnp4th.py:151-198 (custom tanh as "tanh")."""
    kw = hdnnp_model_kwargs(fork)
    local = kw.pop("mlp_kwargs")
    kw.update({
        "mlp_charge_kwargs": {"units": list(fork["charge_hidden"]) + [1], "num_relations": fork["max_elements"],
                              "activation": list(fork["charge_hidden_activation"]) + ["linear"]},
        "mlp_local_kwargs": local,
        "cent_kwargs": {},
        "electrostatic_kwargs": {"name": "electrostatic_layer", "use_physical_params": True, "param_trainable": False},
        "qmmm_kwargs": {"name": "qmmm_layer"},
        "output_embedding": output_embedding,
    })
    return kw


def hdnnp4th_params(seed=12, fork=HDNNP4TH_FORK, random_bias=True):
    """Random weights of the fork's two RelationalMLPs in ``model.weights`` order: the charge network on 640 + 1 inputs
    (symmetry functions and esp), then the local network on 640 + 2 (and the charge)."""
    rng = np.random.default_rng(seed)
    n_el = len(fork["elements"])
    width = len(fork["rs"]) * len(fork["eta"]) * n_el + \
        len(fork["eta_ang"]) * len(fork["zeta"]) * len(fork["lamda"]) * (n_el * (n_el + 1) // 2)
    p = {}
    for net, fan, hidden in (("mlp_charge", width + 1, fork["charge_hidden"]), ("mlp_local", width + 2, fork["hidden"])):
        for k, u in enumerate(list(hidden) + [1]):
            p["%s/%d/kernel" % (net, k)] = glorot_uniform(rng, fan, u, shape=(fork["max_elements"], fan, u))
            p["%s/%d/bias" % (net, k)] = (rng.uniform(-0.1, 0.1, size=u).astype(np.float32) if random_bias
                                          else np.zeros(u, np.float32))
            fan = u
    return p


def _molecule(rng, n, sigma, min_distance):
    """``n`` positions ``N(0, sigma^2)`` in Angstrom, each redrawn until it is ``min_distance`` from the earlier ones."""
    xyz = np.zeros((n, 3))
    for a in range(n):
        while True:
            p = rng.normal(0.0, sigma, size=3)
            if a == 0 or np.min(np.linalg.norm(xyz[:a] - p, axis=-1)) >= min_distance:
                break
        xyz[a] = p
    return xyz


def hdnnp4th_batch(num_graphs=128, seed=4567, sigma=1.5, min_distance=0.9, mixed=False, angles=None, num_mm=12,
                   shell=4.0, fork=HDNNP4TH_FORK, edge_pairing="kj"):
    """HDNNP4th inputs: :func:`hdnnp_batch`'s alanine-dipeptide-shaped molecules (22 atoms, Bohr, range indices by the
    fork's radius, angle indices) plus

    * ``total_charge`` ``(G, 1)`` in {-1, 0, 1};
    * ``num_mm`` MM point charges per molecule, uniform in [-1, 1], on a shell ``shell`` Angstrom outside the molecule's
      farthest atom from its centroid (``mm_positions`` ``(G, num_mm, 3)`` Bohr, ``mm_charges`` ``(G, num_mm)``);
    * ``esp_i = sum_m q_m / |x_i - R_m|`` ``(N,)`` and its gradient ``esp_grad_i = -sum_m q_m (x_i - R_m) / |x_i - R_m|^3``
      ``(N, 3)``, computed in float64 and stored float32.

    ``mixed=True`` cycles the molecule sizes through :data:`MIXED_SIZES` (elements H/C/N/O drawn at random, alanine's
    for 22 atoms) with the spread ``sigma`` scaled by the cube root of the atom count, so that the rejection sampling
    keeps its density and ends.  Angle indices (``angles``, default: not for mixed batches) build an M x M mask per
    molecule and grow cubically with its size: the large molecules serve the charge solve and the electrostatics."""
    rng = np.random.default_rng(seed)
    if angles is None:
        angles = not mixed
    radius = fork["cutoff_rad"] + BOHR_PER_ANGSTROM
    zs, xs, es, ts, qt, mm_x, mm_q, esp, esp_grad = [], [], [], [], [], [], [], [], []
    for g in range(num_graphs):
        n = MIXED_SIZES[g % len(MIXED_SIZES)] if mixed else len(ALANINE_DIPEPTIDE_Z)
        z = ALANINE_DIPEPTIDE_Z if n == len(ALANINE_DIPEPTIDE_Z) else \
            rng.choice(np.array(fork["elements"], np.int64), size=n)
        xyz = _molecule(rng, n, sigma * max(1.0, (n / 22.0) ** (1.0 / 3.0)), min_distance)
        centre = xyz.mean(axis=0)
        r_out = float(np.max(np.linalg.norm(xyz - centre, axis=-1))) + shell
        d = rng.normal(size=(num_mm, 3))
        pos = centre + r_out * d / np.linalg.norm(d, axis=-1, keepdims=True)
        chg = rng.uniform(-1.0, 1.0, size=num_mm)
        xb = (xyz * BOHR_PER_ANGSTROM).astype(np.float32)
        pb = pos * BOHR_PER_ANGSTROM
        diff = xb.astype(np.float64)[:, None, :] - pb[None, :, :]          # (n, m, 3) Bohr
        dist = np.linalg.norm(diff, axis=-1)
        esp.append((chg[None, :] / dist).sum(axis=1).astype(np.float32))
        esp_grad.append((-(chg[None, :, None] * diff) / dist[..., None] ** 3).sum(axis=1).astype(np.float32))
        ei = radius_graph(xb, max_distance=radius, max_neighbours=None)
        zs.append(np.asarray(z, np.int64)); xs.append(xb); es.append(ei)
        ts.append(angle_indices(ei, edge_pairing) if angles else np.zeros((0, 3), np.int64))
        qt.append(float(rng.integers(-1, 2)))
        mm_x.append(pb.astype(np.float32)); mm_q.append(chg.astype(np.float32))
    return {
        "node_number": np.concatenate(zs), "node_coordinates": np.concatenate(xs, axis=0),
        "edge_indices": np.concatenate(es, axis=0).reshape(-1, 2).astype(np.int64),
        "angle_indices": np.concatenate(ts, axis=0).reshape(-1, 3).astype(np.int64),
        "node_splits": _splits([len(x) for x in xs]), "edge_splits": _splits([len(e) for e in es]),
        "angle_splits": _splits([len(t) for t in ts]),
        "total_charge": np.array(qt, np.float32).reshape(-1, 1),
        "esp": np.concatenate(esp), "esp_grad": np.concatenate(esp_grad, axis=0),
        "mm_positions": np.stack(mm_x), "mm_charges": np.stack(mm_q),
    }


# ---------------------------------------------------------------------------------------------------------- DimeNet++
# The model section of the reference's MD17 DimeNet++ force-field runs (training/results/MD17Dataset/
# DimeNetPP_EnergyForceModel/DimeNetPP_hyper_*.json): the energy model inside EnergyForceModel.
DIMENET_MD17 = {
    "name": "DimeNetPPEnergy",
    "inputs": [{"shape": [None], "name": "z", "dtype": "float32", "ragged": True},
               {"shape": [None, 3], "name": "R", "dtype": "float32", "ragged": True},
               {"shape": [None, 2], "name": "range_indices", "dtype": "int64", "ragged": True},
               {"shape": [None, 2], "name": "angle_indices", "dtype": "int64", "ragged": True}],
    "input_embedding": {"node": {"input_dim": 95, "output_dim": 128,
                                 "embeddings_initializer": {"class_name": "RandomUniform",
                                                            "config": {"minval": -1.7320508075688772,
                                                                       "maxval": 1.7320508075688772}}}},
    "emb_size": 128, "out_emb_size": 256, "int_emb_size": 64, "basis_emb_size": 8, "num_blocks": 4,
    "num_spherical": 7, "num_radial": 6, "cutoff": 5.0, "envelope_exponent": 5, "num_before_skip": 1,
    "num_after_skip": 2, "num_dense_output": 3, "num_targets": 1, "extensive": False, "output_init": "zeros",
    "activation": "swish", "verbose": 10, "output_embedding": "graph", "use_output_mlp": False, "output_mlp": {},
}


def angle_pairs(idx, edge_pairing="jk"):
    """Edge pairs ``(n, m)`` forming an angle in one molecule's edge list: the third output of kgcnn/graph/adj.py::
    get_angle_indices with its defaults (no multi, self or reverse edges, sorted).  With "jk", edge ``n = (i, j)`` pairs
    with every ``m = (j, k)``; the pairs are ordered by n, then m."""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1, 2)
    if len(idx) == 0:
        return np.zeros((0, 2), np.int64)
    pos_fix = 1 if edge_pairing[0] == "k" else 0
    pos_ij = 0 if "i" in edge_pairing else 1
    a, b = idx[:, None, :], idx[None, :, :]
    mask = b[..., pos_fix] == a[..., pos_ij]
    mask &= (b[..., 0] != a[..., 0]) | (b[..., 1] != a[..., 1])      # multi edges
    mask &= (b[..., 0] != a[..., 1]) | (b[..., 1] != a[..., 0])      # reverse edges
    np.fill_diagonal(mask, False)                                    # self
    n, m = np.nonzero(mask)
    return np.stack([n, m], axis=-1).astype(np.int64)


def dimenet_batch(num_graphs=64, seed=2345, min_distance=None, sizes=None, max_distance=5.0, **kwargs):
    """``md17_like_batch`` plus the DimeNet++ angle input: ``angle_indices`` (edge pairs of ``angle_pairs``, local to
    each molecule's edge list) and ``angle_splits``.  With ``min_distance`` (or ``sizes``, atoms per molecule) the
    molecules are drawn with no atom pair closer than ``min_distance`` instead (aspirin's elements, cycled)."""
    if min_distance is None and sizes is None:
        b = md17_like_batch(num_graphs=num_graphs, seed=seed, max_distance=max_distance, **kwargs)
    else:
        rng = np.random.default_rng(seed)
        sizes = [21] * num_graphs if sizes is None else list(sizes)
        xs = [_molecule(rng, n, kwargs.get("sigma", 1.7), min_distance or 0.0) for n in sizes]
        es = [radius_graph(x, max_distance=max_distance, max_neighbours=10000).reshape(-1, 2) for x in xs]
        b = {"node_number": np.concatenate([np.resize(ASPIRIN_Z, n) for n in sizes]).astype(np.float32),
             "node_coordinates": np.concatenate(xs, axis=0).astype(np.float32),
             "edge_indices": np.concatenate(es, axis=0).reshape(-1, 2).astype(np.int64),
             "node_splits": _splits(sizes), "edge_splits": _splits([len(e) for e in es])}
    es = b["edge_splits"]
    pairs = [angle_pairs(b["edge_indices"][es[g]:es[g + 1]]) for g in range(len(es) - 1)]
    b["angle_indices"] = np.concatenate(pairs, axis=0).reshape(-1, 2).astype(np.int64)
    b["angle_splits"] = _splits([len(p) for p in pairs])
    return b


def dimenet_params(model, seed=13):
    """Random weights for a built DimeNet++ ``model`` in ``model.weights`` order: Glorot-uniform kernels (the output
    kernels too, which ``output_init="zeros"`` would leave at 0 and the energy identically 0), biases in +-0.1, the
    embedding in +-sqrt(3), Bessel frequencies ``pi * (1..R)``."""
    rng = np.random.default_rng(seed)
    p = {}
    for i, (name, t) in enumerate(model.weights):
        shape = tuple(int(s) for s in t.shape)
        leaf = name.rsplit("/", 1)[-1]
        if leaf == "embeddings":
            v = rng.uniform(-np.sqrt(3.0), np.sqrt(3.0), size=shape)
        elif leaf == "frequencies":
            v = np.pi * np.arange(1, shape[0] + 1)
        elif leaf == "bias":
            v = rng.uniform(-0.1, 0.1, size=shape)
        else:
            v = glorot_uniform(rng, shape[0], shape[-1], shape=shape)
        p["%03d/%s" % (i, name)] = np.asarray(v, dtype=np.float32)
    return p


# --------------------------------------------------------------------------------------------------------------- EGNN
# The model sections of the reference's EGNN runs: training/results/MD17Dataset/EGNN_EnergyForceModel/
# EGNN_hyper_aspirin_ccsd.json (the energy model inside EnergyForceModel) and training/results/QM9Dataset/EGNN/
# EGNN_hyper_U0.json (the same without the position encoding).
EGNN_MD17 = {
    "name": "EGNNEnergy",
    "inputs": [{"shape": [None, 15], "name": "node_attributes", "dtype": "float32", "ragged": True},
               {"shape": [None, 3], "name": "R", "dtype": "float32", "ragged": True},
               {"shape": [None, 2], "name": "range_indices", "dtype": "int64", "ragged": True},
               {"shape": [None, 1], "name": "range_attributes", "dtype": "int64", "ragged": True}],
    "input_embedding": {"node": {"input_dim": 95, "output_dim": 128}, "edge": {"input_dim": 95, "output_dim": 128}},
    "depth": 7,
    "node_mlp_initialize": {"units": 128, "activation": "linear"},
    "euclidean_norm_kwargs": {"keepdims": True, "axis": 2, "square_norm": True},
    "use_edge_attributes": False,
    "edge_mlp_kwargs": {"units": [128, 128], "activation": ["swish", "swish"]},
    "edge_attention_kwargs": {"units": 1, "activation": "sigmoid"},
    "use_normalized_difference": False,
    "expand_distance_kwargs": {"dim_half": 64},
    "coord_mlp_kwargs": None, "pooling_coord_kwargs": None,
    "pooling_edge_kwargs": {"pooling_method": "sum"},
    "node_normalize_kwargs": None, "use_node_attributes": False,
    "node_mlp_kwargs": {"units": [128, 128], "activation": ["swish", "linear"]},
    "use_skip": True, "verbose": 10,
    "node_decoder_kwargs": {"units": [128, 128], "activation": ["swish", "linear"]},
    "node_pooling_kwargs": {"pooling_method": "sum"},
    "output_embedding": "graph", "output_to_tensor": True,
    "output_mlp": {"use_bias": [True, True], "units": [128, 1], "activation": ["swish", "linear"]},
}

EGNN_QM9 = dict(EGNN_MD17, name="EGNN", expand_distance_kwargs=None,
                inputs=[dict(EGNN_MD17["inputs"][0]), dict(EGNN_MD17["inputs"][1], name="node_coordinates"),
                        dict(EGNN_MD17["inputs"][2]), dict(EGNN_MD17["inputs"][3])])


def atomic_charge_representation(numbers, one_hot=(1, 6, 7, 8, 9), charge_scale=9.0, charge_power=2):
    """EGNN's node attributes (the reference's ``atomic_charge_representation`` preprocessor with its defaults): for
    every listed element a block ``[1, z / scale, (z / scale)^2]`` that is zero unless the atom is that element; shape
    ``(N, len(one_hot) * (charge_power + 1))`` float32."""
    z = np.asarray(numbers, dtype=np.float64).reshape(-1)
    out = np.zeros((len(z), len(one_hot), charge_power + 1))
    for j, element in enumerate(one_hot):
        rows = z == element
        for p in range(charge_power + 1):
            out[rows, j, p] = (z[rows] / charge_scale) ** p
    return out.reshape(len(z), -1).astype(np.float32)


def egnn_batch(num_graphs=64, seed=2345, min_distance=0.9, sizes=None, max_distance=10.0, sigma=1.7):
    """MD17-shaped EGNN inputs: aspirin-composition molecules (21 atoms, or ``sizes`` atoms each with aspirin's elements
    cycled) with no atom pair closer than ``min_distance``, ``node_attributes`` (N, 15) of
    :func:`atomic_charge_representation`, and every pair within ``max_distance`` as a directed edge (10 A in the
    reference's runs: the graphs are fully connected)."""
    rng = np.random.default_rng(seed)
    sizes = [21] * num_graphs if sizes is None else list(sizes)
    xs = [_molecule(rng, n, sigma, min_distance or 0.0) for n in sizes]
    es = [radius_graph(x, max_distance=max_distance, max_neighbours=10000).reshape(-1, 2) for x in xs]
    numbers = np.concatenate([np.resize(ASPIRIN_Z, n) for n in sizes]).astype(np.float32) if sizes else \
        np.zeros(0, np.float32)
    return {"node_number": numbers, "node_attributes": atomic_charge_representation(numbers),
            "node_coordinates": np.concatenate(xs, axis=0).astype(np.float32).reshape(-1, 3),
            "edge_indices": np.concatenate(es, axis=0).reshape(-1, 2).astype(np.int64),
            "node_splits": _splits(sizes), "edge_splits": _splits([len(e) for e in es])}


def egnn_params(model, seed=14):
    """Random weights for a built EGNN ``model`` in ``model.weights`` order: Glorot-uniform kernels, biases in +-0.1,
    embeddings in +-0.05."""
    rng = np.random.default_rng(seed)
    p = {}
    for i, (name, t) in enumerate(model.weights):
        shape = tuple(int(s) for s in t.shape)
        leaf = name.rsplit("/", 1)[-1]
        if leaf == "embeddings":
            v = rng.uniform(-0.05, 0.05, size=shape)
        elif leaf == "bias":
            v = rng.uniform(-0.1, 0.1, size=shape)
        else:
            v = glorot_uniform(rng, shape[0], shape[-1], shape=shape)
        p["%03d/%s" % (i, name)] = np.asarray(v, dtype=np.float32)
    return p


def periodic_structures(num_graphs=128, seed=5678, min_atoms=4, max_atoms=30, density=0.07, skew=0.1):
    """Random periodic structures for the periodic-cell measurements: per structure ``n`` atoms (uniform in
    ``[min_atoms, max_atoms]``) at uniform fractional positions in a cell of volume about ``n / density`` (atoms per
    cubic Angstrom; 0.07 is typical of inorganic crystals), ``edge * (I + skew * uniform(-1, 1, (3, 3)))`` with the
    lattice vectors in rows.  Returns ``node_number`` (int64), ``node_coordinates`` (float32), ``node_splits`` and
    ``graph_lattice`` ``(G, 3, 3)`` float32."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(min_atoms, max_atoms + 1, size=num_graphs)
    numbers, coords, lattices = [], [], []
    for n in sizes:
        edge = (float(n) / density) ** (1.0 / 3.0)
        lat = edge * (np.eye(3) + skew * rng.uniform(-1.0, 1.0, size=(3, 3)))
        coords.append((rng.uniform(0.0, 1.0, size=(int(n), 3)) @ lat).astype(np.float32))
        lattices.append(lat.astype(np.float32))
        numbers.append(rng.choice(np.array([1, 6, 7, 8, 14], dtype=np.int64), size=int(n)))
    return {"node_number": np.concatenate(numbers), "node_coordinates": np.concatenate(coords, axis=0),
            "node_splits": _splits(sizes), "graph_lattice": np.stack(lattices)}


def cgcnn_batch(structures=None, edges=None, **kwargs):
    """CGCNN inputs of periodic structures: ``structures`` is a batch of :func:`periodic_structures` (made with
    ``kwargs`` when left out).  Adds ``node_frac_coordinates`` (float32; ``x L^-1`` with the float64 inverse of the
    float32 lattice) and ``lattice_matrix``, the lattice TRANSPOSED - the convention ``FracToRealCoordinates`` computes
    with (``A f``, see literature/CGCNN.py).  ``edges``: a dict with ``edge_indices`` (or ``range_indices``),
    ``edge_image`` (or ``range_image``) and ``edge_splits`` from a neighbour search (``SetRangePeriodic``, or a brute
    force) - copied in as ``edge_indices``, ``cell_translations`` (float32) and ``edge_splits``."""
    b = dict(periodic_structures(**kwargs) if structures is None else structures)
    ns, lat = np.asarray(b["node_splits"]), np.asarray(b["graph_lattice"], dtype=np.float64)
    xyz = np.asarray(b["node_coordinates"], dtype=np.float64).reshape(-1, 3)
    frac = np.zeros_like(xyz)
    for g in range(len(ns) - 1):
        frac[ns[g]:ns[g + 1]] = xyz[ns[g]:ns[g + 1]] @ np.linalg.inv(lat[g])
    b["node_frac_coordinates"] = frac.astype(np.float32)
    b["lattice_matrix"] = np.ascontiguousarray(np.transpose(lat, (0, 2, 1))).astype(np.float32)
    if edges is not None:
        idx = edges["edge_indices"] if "edge_indices" in edges else edges["range_indices"]
        img = edges["edge_image"] if "edge_image" in edges else edges["range_image"]
        b["edge_indices"] = np.asarray(idx, dtype=np.int64).reshape(-1, 2)
        b["cell_translations"] = np.asarray(img).reshape(-1, 3).astype(np.float32)
        b["edge_splits"] = np.asarray(edges["edge_splits"], dtype=np.int64)
    return b


def cgcnn_params(model, seed=31):
    """Random weights for a built CGCNN ``model`` in ``model.weights`` order: Glorot-uniform kernels, biases in +-0.1,
    embeddings in +-0.05, and non-trivial batch-norm vectors (gamma in [0.5, 1.5], beta in +-0.3, moving mean in +-0.5,
    moving variance in [0.5, 2])."""
    rng = np.random.default_rng(seed)
    draw = {"embeddings": (-0.05, 0.05), "bias": (-0.1, 0.1), "gamma": (0.5, 1.5), "beta": (-0.3, 0.3),
            "moving_mean": (-0.5, 0.5), "moving_variance": (0.5, 2.0)}
    p = {}
    for i, (name, t) in enumerate(model.weights):
        shape = tuple(int(s) for s in t.shape)
        leaf = name.rsplit("/", 1)[-1]
        if leaf in draw:
            v = rng.uniform(draw[leaf][0], draw[leaf][1], size=shape)
        else:
            v = glorot_uniform(rng, shape[0], shape[-1], shape=shape)
        p["%03d/%s" % (i, name)] = np.asarray(v, dtype=np.float32)
    return p


def cmpnn_batch(num_graphs=128, seed=6789, min_atoms=6, max_atoms=19, max_rings=3, node_types=10, edge_types=4,
                node_features=12, edge_features=8):
    """Molecule-like graphs for CMPNN / DMPNN: per graph a random tree over ``n`` atoms (uniform in ``[min_atoms,
    max_atoms]``) plus up to ``max_rings`` ring-closing bonds, every bond in both directions, the directed edges sorted by
    (receiver, sender).  ``edge_indices_reverse`` ``(M, 1)`` holds, per edge, the position of its reverse edge in the
    graph's own list.  Integer ``node_number`` (1..``node_types``) and ``edge_number`` (1..``edge_types``, equal for both
    directions of a bond) feed the embedding inputs; ``node_attributes`` / ``edge_attributes`` are float32 features, normal
    times 0.3, for the feature inputs."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(min_atoms, max_atoms + 1, size=num_graphs)
    idx, rev, etype, counts = [], [], [], []
    for n in sizes:
        n = int(n)
        bonds = {(int(rng.integers(0, a)), a) for a in range(1, n)}
        for _ in range(int(rng.integers(0, max_rings + 1))):
            a, b = (int(v) for v in rng.choice(n, size=2, replace=False))
            bonds.add((min(a, b), max(a, b)))
        kind = {bond: int(rng.integers(1, edge_types + 1)) for bond in sorted(bonds)}
        directed = sorted([(a, b) for a, b in bonds] + [(b, a) for a, b in bonds])
        where = {e: i for i, e in enumerate(directed)}
        idx.append(np.array(directed, dtype=np.int64).reshape(-1, 2))
        rev.append(np.array([where[(b, a)] for a, b in directed], dtype=np.int64).reshape(-1, 1))
        etype.append(np.array([kind[(min(a, b), max(a, b))] for a, b in directed], dtype=np.int64))
        counts.append(len(directed))
    n_total, m_total = int(np.sum(sizes)), int(np.sum(counts))
    return {"node_number": rng.integers(1, node_types + 1, size=n_total).astype(np.int64),
            "edge_number": np.concatenate(etype),
            "node_attributes": (0.3 * rng.normal(size=(n_total, node_features))).astype(np.float32),
            "edge_attributes": (0.3 * rng.normal(size=(m_total, edge_features))).astype(np.float32),
            "edge_indices": np.concatenate(idx, axis=0), "edge_indices_reverse": np.concatenate(rev, axis=0),
            "node_splits": _splits(sizes), "edge_splits": _splits(counts)}


def cmpnn_params(model, seed=41, dense_scale=0.5):
    """Random weights for a built CMPNN ``model`` in ``model.weights`` order: Dense kernels Glorot-uniform times
    ``dense_scale``, the GRU's two kernels full Glorot-uniform, biases in +-0.1, embeddings in +-0.5.  The booster
    multiplies a sum by a max, so states grow quadratically per round: with full-scale Dense kernels they reach 1e3-1e5
    after four rounds and float32 pipelines part by 1e-5; half scale keeps them O(1)."""
    rng = np.random.default_rng(seed)
    p = {}
    for i, (name, t) in enumerate(model.weights):
        shape = tuple(int(s) for s in t.shape)
        leaf = name.rsplit("/", 1)[-1]
        if leaf == "embeddings":
            v = rng.uniform(-0.5, 0.5, size=shape)
        elif leaf == "bias":
            v = rng.uniform(-0.1, 0.1, size=shape)
        elif "gru_cell" in name:
            v = glorot_uniform(rng, shape[0], shape[-1], shape=shape)
        else:
            v = dense_scale * glorot_uniform(rng, shape[0], shape[-1], shape=shape)
        p["%03d/%s" % (i, name)] = np.asarray(v, dtype=np.float32)
    return p


def attentivefp_params(model, seed=47, dense_scale=1.0):
    """Random weights for a built AttentiveFP ``model`` in ``model.weights`` order (``cmpnn_params``' rules: Dense kernels
    Glorot-uniform times ``dense_scale``, the GRU cells' kernels full Glorot-uniform, biases in +-0.1, embeddings in
    +-0.5).  ``cmpnn_batch`` gives the bond graphs, with integer types for the embedding inputs and float features."""
    return cmpnn_params(model, seed=seed, dense_scale=dense_scale)


def relational_batch(num_graphs=128, seed=7890, num_relations=20, **kwargs):
    """``cmpnn_batch`` graphs for RGCN / GNNFilm: additionally ``edge_relations`` ``(M,)`` int64, uniform in
    ``[0, num_relations)`` and equal for both directions of a bond, and ``edge_weights`` ``(M, 1)`` float32 in
    ``[0.25, 1.25)``."""
    b = cmpnn_batch(num_graphs, seed=seed, **kwargs)
    rng = np.random.default_rng(seed + 1)
    m = len(b["edge_indices"])
    relations = np.zeros(m, dtype=np.int64)
    es = b["edge_splits"]
    for g in range(num_graphs):
        lo, hi = int(es[g]), int(es[g + 1])
        idx, rev = b["edge_indices"][lo:hi], b["edge_indices_reverse"][lo:hi, 0]
        draw = rng.integers(0, num_relations, size=hi - lo)
        forward = idx[:, 0] < idx[:, 1]
        relations[lo:hi] = np.where(forward, draw, draw[rev])
    b["edge_relations"] = relations
    b["edge_weights"] = rng.uniform(0.25, 1.25, size=(m, 1)).astype(np.float32)
    return b


def relational_params(model, seed=43, dense_scale=1.0):
    """Random weights for a built RGCN / GNNFilm ``model`` in ``model.weights`` order: every kernel Glorot-uniform on its
    last two axes times ``dense_scale`` (a relation's, a basis' or a block's own fan), ``lin_bases`` Glorot-uniform, biases
    in +-0.1, embeddings in +-0.5."""
    rng = np.random.default_rng(seed)
    p = {}
    for i, (name, t) in enumerate(model.weights):
        shape = tuple(int(s) for s in t.shape)
        leaf = name.rsplit("/", 1)[-1]
        if leaf == "embeddings":
            v = rng.uniform(-0.5, 0.5, size=shape)
        elif leaf == "bias":
            v = rng.uniform(-0.1, 0.1, size=shape)
        else:
            v = dense_scale * glorot_uniform(rng, shape[-2], shape[-1], shape=shape)
        p["%03d/%s" % (i, name)] = np.asarray(v, dtype=np.float32)
    return p


def megan_batch(num_graphs=128, seed=1234, node_features=12, edge_features=6, **kwargs):
    """MEGAN inputs on the :func:`qm9_like_batch` graphs (``kwargs`` go there): additionally ``node_attributes``
    ``(N, node_features)`` and ``edge_attributes`` ``(M, edge_features)``, float32 ``N(0, 1)`` from a stream of their own
    (``seed + 2``), and ``node_type`` ``(N,)`` float32 numbers in ``[0, 95)`` for an embedding input."""
    b = qm9_like_batch(num_graphs=num_graphs, seed=seed, **kwargs)
    rng = np.random.default_rng(seed + 2)
    n, m = int(b["node_splits"][-1]), int(b["edge_splits"][-1])
    b["node_attributes"] = rng.normal(size=(n, node_features)).astype(np.float32)
    b["edge_attributes"] = rng.normal(size=(m, edge_features)).astype(np.float32)
    b["node_type"] = rng.integers(0, 95, size=n).astype(np.float32)
    return b


def megan_params(model, seed=53, dense_scale=1.0):
    """Random weights for a built MEGAN ``model`` in ``model.weights`` order: kernels Glorot-uniform times ``dense_scale``,
    biases in +-0.1, embeddings in +-0.5.  At scale 1 the summed attention logits stay of order 1, so the edge
    importances do not saturate."""
    return relational_params(model, seed=seed, dense_scale=dense_scale)


def mat_batch(num_graphs=128, seed=9012, sigma=1.6, min_distance=0.9, **kwargs):
    """MAT inputs on the :func:`cmpnn_batch` bond graphs (``kwargs`` go there): additionally ``node_coordinates``
    ``(N, 3)`` float32 from :func:`_molecule` (Angstrom, ``min_distance`` apart) and ``edge_weights`` ``(M, 1)`` float32,
    a bond order in {1, 1.5, 2, 3} equal for both directions of a bond; ``node_number`` is float32 for the embedding
    input."""
    b = cmpnn_batch(num_graphs, seed=seed, **kwargs)
    rng = np.random.default_rng(seed + 3)
    ns, es = b["node_splits"], b["edge_splits"]
    b["node_coordinates"] = np.concatenate(
        [_molecule(rng, int(ns[g + 1] - ns[g]), sigma, min_distance) for g in range(num_graphs)]
        + [np.zeros((0, 3))], axis=0).astype(np.float32)
    orders = np.array([1.0, 1.5, 2.0, 3.0], dtype=np.float32)
    weights = np.zeros((int(es[-1]), 1), dtype=np.float32)
    for g in range(num_graphs):
        lo, hi = int(es[g]), int(es[g + 1])
        idx, rev = b["edge_indices"][lo:hi], b["edge_indices_reverse"][lo:hi, 0]
        draw = orders[rng.integers(0, 4, size=hi - lo)]
        weights[lo:hi, 0] = np.where(idx[:, 0] < idx[:, 1], draw, draw[rev])
    b["edge_weights"] = weights
    b["node_number"] = b["node_number"].astype(np.float32)
    return b


def mat_params(model, seed=59, dense_scale=0.5):
    """Random weights for a built MAT ``model`` in ``model.weights`` order (``cmpnn_params``' rules: Dense kernels
    Glorot-uniform times ``dense_scale``, biases in +-0.1, embeddings in +-0.5); the layer normalisations' ``gamma`` in
    ``1 +- 0.1`` and ``beta`` in ``+-0.1``, so that neither is the identity."""
    rng = np.random.default_rng(seed)
    p = cmpnn_params(model, seed=seed, dense_scale=dense_scale)
    for key in p:
        leaf = key.rsplit("/", 1)[-1]
        if leaf in ("gamma", "beta"):
            p[key] = ((1.0 if leaf == "gamma" else 0.0) + rng.uniform(-0.1, 0.1, size=p[key].shape)).astype(np.float32)
    return p


def unet_batch(num_graphs=128, seed=7, node_features=12, **kwargs):
    """Graph U-Net inputs on the :func:`cmpnn_batch` bond graphs (``kwargs`` go there): ``node_attributes``
    ``(N, node_features)`` float32 ``N(0, 1)`` (continuous, so that scores differ unless rows are bit-equal) and
    ``edge_weights`` ``(M, 1)`` float32 ``0.5 + |0.3 N(0, 1)|`` from a stream of their own (``seed + 4``): positive
    adjacency weights in column 0, which keep every entry of ``A^2`` far above the Keras epsilon at every level (with the
    Keras default edge embedding, +-0.05, the entries fall below 1e-7 by the third level and every edge goes).
    ``node_number`` and ``edge_number`` are float32 for the embedding inputs of the default model.

    The pooled structure is a discontinuous function of the scores and of the threshold, so a comparison against another
    implementation needs inputs on which near-ties and near-threshold entries do not occur; tests/test_unet_api.py
    asserts that for ``unet_batch(12)`` with ``unet_params`` (the default seeds were searched for it)."""
    b = cmpnn_batch(num_graphs, seed=seed, **kwargs)
    rng = np.random.default_rng(seed + 4)
    n, m = int(b["node_splits"][-1]), int(b["edge_splits"][-1])
    b["node_attributes"] = rng.normal(size=(n, node_features)).astype(np.float32)
    b["edge_weights"] = (0.5 + np.abs(0.3 * rng.normal(size=(m, 1)))).astype(np.float32)
    b["node_number"] = b["node_number"].astype(np.float32)
    b["edge_number"] = b["edge_number"].astype(np.float32)
    return b


def unet_params(model, seed=61, dense_scale=1.3):
    """Random weights for a built Graph U-Net ``model`` in ``model.weights`` order: Dense kernels Glorot-uniform times
    ``dense_scale``, biases in +-0.1, the pooling scores in ``1 +- 0.2``, a node embedding in +-0.5 and an edge embedding
    ``0.5 + |0.3 N(0, 1)|`` (positive adjacency weights, see :func:`unet_batch`).  At scale 1.3 the default model's
    outputs spread over 0.2 .. 0.5; at 2 the nine convolutions drive the output sigmoid into saturation."""
    rng = np.random.default_rng(seed)
    p = {}
    tables = [i for i, (name, _) in enumerate(model.weights) if name.rsplit("/", 1)[-1] == "embeddings"]
    edge_table = tables[-1] if tables and model.config.get("edge_input_dim") is not None else -1
    for i, (name, t) in enumerate(model.weights):
        shape = tuple(int(s) for s in t.shape)
        leaf = name.rsplit("/", 1)[-1]
        if leaf == "embeddings":
            edge = i == edge_table
            v = 0.5 + np.abs(0.3 * rng.normal(size=shape)) if edge else rng.uniform(-0.5, 0.5, size=shape)
        elif leaf == "bias":
            v = rng.uniform(-0.1, 0.1, size=shape)
        elif leaf == "score":
            v = 1.0 + rng.uniform(-0.2, 0.2, size=shape)
        else:
            v = dense_scale * glorot_uniform(rng, shape[0], shape[-1], shape=shape)
        p["%03d/%s" % (i, name)] = np.asarray(v, dtype=np.float32)
    return p


# ------------------------------------------------------------------------------------------------------------- MXMNet
# The model section of the reference's MD17 MXMNet force-field runs (training/results/MD17Dataset/
# MXMNet_EnergyForceModel/MXMNet_hyper_*.json): the energy model inside EnergyForceModel.  Local edges: the 3 A range
# graph; global edges: the 5 A range graph.
MXMNET_MD17 = {
    "name": "MXMNetEnergy",
    "inputs": [{"shape": [None], "name": "z", "dtype": "float32", "ragged": True},
               {"shape": [None, 3], "name": "R", "dtype": "float32", "ragged": True},
               {"shape": [None, 1], "name": "edge_weights", "dtype": "float32", "ragged": True},
               {"shape": [None, 2], "name": "edge_indices", "dtype": "int64", "ragged": True},
               {"shape": [None, 2], "name": "angle_indices_1", "dtype": "int64", "ragged": True},
               {"shape": [None, 2], "name": "angle_indices_2", "dtype": "int64", "ragged": True},
               {"shape": [None, 2], "name": "range_indices", "dtype": "int64", "ragged": True}],
    "input_embedding": {"node": {"input_dim": 95, "output_dim": 128,
                                 "embeddings_initializer": {"class_name": "RandomUniform",
                                                            "config": {"minval": -1.7320508075688772,
                                                                       "maxval": 1.7320508075688772}}},
                        "edge": {"input_dim": 32, "output_dim": 128}},
    "bessel_basis_local": {"num_radial": 16, "cutoff": 5.0, "envelope_exponent": 5},
    "bessel_basis_global": {"num_radial": 16, "cutoff": 5.0, "envelope_exponent": 5},
    "spherical_basis_local": {"num_spherical": 7, "num_radial": 6, "cutoff": 5.0, "envelope_exponent": 5},
    "mlp_rbf_kwargs": {"units": 128, "activation": "swish"}, "mlp_sbf_kwargs": {"units": 128, "activation": "swish"},
    "global_mp_kwargs": {"units": 128},
    "local_mp_kwargs": {"units": 128, "output_units": 1, "output_kernel_initializer": "zeros"},
    "use_edge_attributes": False, "depth": 6, "verbose": 10, "node_pooling_args": {"pooling_method": "sum"},
    "output_embedding": "graph", "output_to_tensor": True, "use_output_mlp": False,
    "output_mlp": {"use_bias": [True], "units": [1], "activation": ["linear"]},
}


def angle_pairs_ik_self(idx):
    """Edge pairs ``(n, m)`` of kgcnn/graph/adj.py::get_angle_indices with ``edge_pairing="ik"`` and
    ``allow_self_edges=True`` (MXMNet's second angle list): edge ``n = (i, j)`` pairs with every ``m = (i, k)``, no multi
    or reverse edges, and with itself; ordered by n, then m."""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1, 2)
    if len(idx) == 0:
        return np.zeros((0, 2), np.int64)
    a, b = idx[:, None, :], idx[None, :, :]
    mask = b[..., 0] == a[..., 0]
    mask &= (b[..., 0] != a[..., 0]) | (b[..., 1] != a[..., 1])      # multi edges
    mask &= (b[..., 0] != a[..., 1]) | (b[..., 1] != a[..., 0])      # reverse edges
    np.fill_diagonal(mask, True)                                     # self
    n, m = np.nonzero(mask)
    return np.stack([n, m], axis=-1).astype(np.int64)


def mxmnet_batch(num_graphs=64, seed=2345, min_distance=0.9, sizes=None, local_distance=3.0, range_distance=5.0,
                 sigma=1.7):
    """A batch of MXMNet's seven inputs: molecules of ``sizes`` atoms (default 21, aspirin's elements cycled) drawn as
    :func:`_molecule` draws them, the local edges within ``local_distance`` with both angle lists (``angle_indices_1``:
    :func:`angle_pairs` "jk"; ``angle_indices_2``: :func:`angle_pairs_ik_self`), the global edges within
    ``range_distance`` and uniform edge weights ``(E, 1)``; every index list is local to its molecule."""
    rng = np.random.default_rng(seed)
    sizes = [21] * num_graphs if sizes is None else list(sizes)
    xs = [_molecule(rng, n, sigma, min_distance) for n in sizes]
    es = [radius_graph(x, max_distance=local_distance, max_neighbours=10000).reshape(-1, 2) for x in xs]
    rs = [radius_graph(x, max_distance=range_distance, max_neighbours=10000).reshape(-1, 2) for x in xs]
    a1 = [angle_pairs(e, "jk") for e in es]
    a2 = [angle_pairs_ik_self(e) for e in es]

    def cat(parts, width):
        return np.concatenate(parts, axis=0).reshape(-1, width).astype(np.int64)

    b = {"node_number": np.concatenate([np.resize(ASPIRIN_Z, n) for n in sizes] or [np.zeros(0)]).astype(np.float32),
         "node_coordinates": np.concatenate(xs, axis=0).reshape(-1, 3).astype(np.float32),
         "edge_indices": cat(es, 2), "range_indices": cat(rs, 2),
         "angle_indices_1": cat(a1, 2), "angle_indices_2": cat(a2, 2),
         "node_splits": _splits(sizes), "edge_splits": _splits([len(e) for e in es]),
         "range_splits": _splits([len(r) for r in rs]), "angle_splits_1": _splits([len(a) for a in a1]),
         "angle_splits_2": _splits([len(a) for a in a2])}
    b["edge_weights"] = np.ones((len(b["edge_indices"]), 1), dtype=np.float32)
    return b


def mxmnet_params(model, seed=17, dense_scale=0.6):
    """Random weights for a built MXMNet ``model`` in ``model.weights`` order: Dense kernels Glorot-uniform times
    ``dense_scale`` (the output kernels too, which ``output_kernel_initializer="zeros"`` would leave at 0 and the output
    a constant), biases in +-0.1, the embedding in +-sqrt(3), Bessel frequencies ``pi * (1..R)``.  The local message
    passing sums over edges and triplets without a normalisation: at scale 1 the node states of a 9-atom molecule grow
    by orders of magnitude per block, and float32 forces lose their digits whoever computes them."""
    rng = np.random.default_rng(seed)
    p = {}
    for i, (name, t) in enumerate(model.weights):
        shape = tuple(int(s) for s in t.shape)
        leaf = name.rsplit("/", 1)[-1]
        if leaf == "embeddings":
            v = rng.uniform(-np.sqrt(3.0), np.sqrt(3.0), size=shape)
        elif leaf == "frequencies":
            v = np.pi * np.arange(1, shape[0] + 1)
        elif leaf == "bias":
            v = rng.uniform(-0.1, 0.1, size=shape)
        else:
            v = dense_scale * glorot_uniform(rng, shape[0], shape[-1], shape=shape)
        p["%03d/%s" % (i, name)] = np.asarray(v, dtype=np.float32)
    return p
