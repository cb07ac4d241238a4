"""Differentiable torch-CPU restatement of MXMNet (kgcnn/literature/MXMNet.py:122-185 and the two layers of
kgcnn/layers/conv/mxmnet_conv.py), in float64 or float32: the budget and the float32 twin of the GPU tests.  Forces come
from autograd.  The Bessel and spherical bases are those of tests/dimenet_reference.py.

Weights are looked up by the engine layer's attribute (``layer.h_mlp``, ``layer.linear`` ...), not by their position in
``model.weights``: ``weights_of(obj, arrays)`` maps every weight tensor of a layer or model to the array at its position
and the restatement asks that table for ``dense.kernel`` / ``dense.bias``.  The order of ``model.weights`` therefore does
not enter the comparison.

``angle_lists`` builds both angle lists of one molecule from their definitions (kgcnn/graph/adj.py::get_angle_indices):
pairing "jk" without self pairs and pairing "ik" WITH the self pairs ``(n, n)``.  With ``vector_scale=[1, -1]`` a self
pair's angle is that of ``v`` and ``-v``, the constant pi; the engine gives it a zero gradient (the collinear rule of
mp_edge_angle_grad_f32), and the restatement writes the constant there, too, rather than differentiate ``atan2`` at a
zero cross product.
"""
import math

import numpy as np
import torch

import dimenet_reference as dref

ACTIVATIONS = {
    "swish": dref.swish, "kgcnn>swish": dref.swish, "linear": lambda x: x, None: lambda x: x,
    "relu": torch.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid, "softplus": torch.nn.functional.softplus,
}


# ------------------------------------------------------------------------------------------------ angle lists
def angle_lists(idx):
    """``(pairs_jk, pairs_ik_self)`` of one molecule's edge list ``(E, 2)``, each ``(T, 2)`` int64 of edge positions
    ``(n, m)`` ordered by n, then m.  Edge ``n = (i, j)``:

    * "jk": every edge ``m = (j, k)`` that is not ``n``, has not n's node pair and is not its reverse ``(j, i)``;
    * "ik" with self pairs: every edge ``m = (i, k)`` that has not n's node pair and is not its reverse, and ``n``."""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1, 2)
    jk, ik = [], []
    for n, (i, j) in enumerate(idx):
        for m, (a, b) in enumerate(idx):
            same, reverse = (a == i and b == j), (a == j and b == i)
            if a == j and m != n and not same and not reverse:
                jk.append((n, m))
            if m == n or (a == i and not same and not reverse):
                ik.append((n, m))
    return (np.asarray(jk, dtype=np.int64).reshape(-1, 2), np.asarray(ik, dtype=np.int64).reshape(-1, 2))


def flat_indices(b):
    """Flat (batch-shifted) edge, range and angle indices of a synth.mxmnet_batch: ``(ei, ri, a1, a2)``."""
    ns, es, rs = b["node_splits"], b["edge_splits"], b["range_splits"]
    ei, ri = b["edge_indices"].copy(), b["range_indices"].copy()
    a1, a2 = b["angle_indices_1"].copy(), b["angle_indices_2"].copy()
    s1, s2 = b["angle_splits_1"], b["angle_splits_2"]
    for g in range(len(ns) - 1):
        ei[es[g]:es[g + 1]] += ns[g]
        ri[rs[g]:rs[g + 1]] += ns[g]
        a1[s1[g]:s1[g + 1]] += es[g]
        a2[s2[g]:s2[g + 1]] += es[g]
    return ei, ri, a1, a2


# ------------------------------------------------------------------------------------------------ weights, pieces
def weights_of(obj, arrays):
    """``id(weight tensor) -> array`` for the weights of a layer or model, ``arrays`` in ``obj.weights`` order."""
    ws = obj.weights
    assert len(ws) == len(arrays), (len(ws), len(arrays))
    return {id(t): np.asarray(a) for (_, t), a in zip(ws, arrays)}


class _Net:
    """The pieces of the restatement over one weight table and dtype."""

    def __init__(self, table, dtype):
        self.table, self.dtype = table, dtype

    def w(self, t):
        return torch.tensor(self.table[id(t)], dtype=self.dtype)

    def dense(self, layer, x, activation=None):
        y = x @ self.w(layer.kernel)
        if layer.bias is not None:
            y = y + self.w(layer.bias)
        act = layer.activation if activation is None else activation
        return ACTIVATIONS[act](y)

    def mlp(self, layer, x):
        for d, a in zip(layer.mlp_dense_layer_list, layer.mlp_activation_layer_list):
            x = self.dense(d, x, activation=a.activation)
        return x

    def residual(self, layer, x):
        return x + self.dense(layer.dense_2, self.dense(layer.dense_1, x))

    @staticmethod
    def pool(x, idx, rows, method):
        out = torch.zeros((rows,) + tuple(x.shape[1:]), dtype=x.dtype).index_add(0, idx, x)
        if method == "mean":
            count = torch.zeros(rows, dtype=x.dtype).index_add(0, idx, torch.ones(len(idx), dtype=x.dtype))
            out = out / count.clamp(min=1)[:, None]
        return out

    # -- kgcnn/layers/conv/mxmnet_conv.py:38-53
    def propagate(self, layer, x, a, ri):
        x_edge = self.mlp(layer.x_edge_mlp, torch.cat([x[ri[:, 0]], x[ri[:, 1]], a], dim=-1))
        x_edge = self.dense(layer.linear, a) * x_edge
        return self.pool(x_edge, ri[:, 0], x.shape[0], layer.pool.pooling_method) + x

    # -- kgcnn/layers/conv/mxmnet_conv.py:55-77
    def global_mp(self, layer, h, a, ri):
        res_h = h
        h = self.mlp(layer.h_mlp, h)
        h = self.propagate(layer, h, a, ri)
        h = self.residual(layer.res1, h)
        h = self.mlp(layer.mlp, h) + res_h
        h = self.residual(layer.res2, h)
        h = self.residual(layer.res3, h)
        return self.propagate(layer, h, a, ri)

    # -- kgcnn/layers/conv/mxmnet_conv.py:131-183
    def local_mp(self, layer, h, rbf, sbf1, sbf2, ei, a1, a2):
        method, n_edges = layer.pooling_method, int(ei.shape[0])
        res_h = h
        h = self.mlp(layer.h_mlp, h)
        m = torch.cat([h[ei[:, 0]], h[ei[:, 1]], rbf], dim=-1)

        m_kj = self.mlp(layer.mlp_kj, m) * self.dense(layer.lin_rbf1, rbf)
        m_kj = m_kj[a1[:, 1]] * self.mlp(layer.mlp_sbf1, sbf1)
        m_kj = self.pool(m_kj, a1[:, 0], n_edges, method)
        m = self.mlp(layer.mlp_ji_1, m) + m_kj

        m_jj = self.mlp(layer.mlp_jj, m) * self.dense(layer.lin_rbf2, rbf)
        m_jj = m_jj[a2[:, 1]] * self.mlp(layer.mlp_sbf2, sbf2)
        m_jj = self.pool(m_jj, a2[:, 0], n_edges, method)
        m = self.mlp(layer.mlp_ji_2, m) + m_jj

        m = self.dense(layer.lin_rbf_out, rbf) * m
        h = self.pool(m, ei[:, 0], h.shape[0], method)

        h = self.residual(layer.res1, h)
        h = self.mlp(layer.h_mlp, h) + res_h
        h = self.residual(layer.res2, h)
        h = self.residual(layer.res3, h)
        return h, self.dense(layer.y_W, self.mlp(layer.y_mlp, h))


def global_mp(layer, weights, h, a, ri, dtype=torch.float64):
    """``MXMGlobalMP`` on flat tensors: ``h`` (N, F), ``a`` (E, Ka), ``ri`` (E, 2) long."""
    return _Net(weights_of(layer, weights), dtype).global_mp(layer, h, a, ri)


def propagate(layer, weights, x, a, ri, dtype=torch.float64):
    return _Net(weights_of(layer, weights), dtype).propagate(layer, x, a, ri)


def local_mp(layer, weights, h, rbf, sbf1, sbf2, ei, a1, a2, dtype=torch.float64):
    """``MXMLocalMP`` on flat tensors; returns ``(h, y)``."""
    return _Net(weights_of(layer, weights), dtype).local_mp(layer, h, rbf, sbf1, sbf2, ei, a1, a2)


def edge_message(x, a, idx, kernel, bias, wl, activation, method=None, base=None):
    """The multiplex edge message on flat tensors, op for op as the layers spell it: ``act([x_i || x_j || a] kernel +
    bias) * (a wl)`` (``wl`` None: no gate), per edge ``(E, W)`` with ``method`` None, else pooled into column 0 by
    ``method`` with ``base`` (None: nothing) added."""
    y = torch.cat([x[idx[:, 0]], x[idx[:, 1]], a], dim=-1) @ kernel
    if bias is not None:
        y = y + bias
    y = ACTIVATIONS[activation](y)
    if wl is not None:
        y = (a @ wl) * y
    if method is None:
        return y
    out = _Net.pool(y, idx[:, 0], x.shape[0], method)
    return out if base is None else out + base


def triplet_pool(x, s, pairs, method):
    """``pool_{t: A[t,0] = n} x[A[t,1]] * s[t]`` over the E rows of ``x``."""
    return _Net.pool(x[pairs[:, 1]] * s, pairs[:, 0], x.shape[0], method)


# ------------------------------------------------------------------------------------------------ shared test cases
MODEL_SIZES = [3, 4, 5, 6, 7, 9]   # atoms per molecule of the whole-model tests
WEIGHT_SEED = 3                    # synth.mxmnet_params seed of the whole-model tests


def model_config(which, synth, MXMNet):
    """The two model configurations of the tests, their output kernels Glorot-uniform (``"zeros"`` would make every
    output a constant): ``"default"`` = ``model_default`` (width 32, depth 3), ``"md17"`` = the reference's MD17
    configuration (width 128) at depth 2."""
    cfg = dict(MXMNet.model_default) if which == "default" else dict(synth.MXMNET_MD17, depth=2)
    cfg["local_mp_kwargs"] = dict(cfg["local_mp_kwargs"], output_kernel_initializer="glorot_uniform")
    return cfg


def model_batch(which, synth):
    """6 molecules of 3 to 9 atoms, no pair closer than 0.9 A; local edges within 3 A (md17) or 2 A (default), range
    edges within 5 A."""
    return synth.mxmnet_batch(sizes=MODEL_SIZES, seed=21 if which == "default" else 22, min_distance=0.9,
                              local_distance=2.0 if which == "default" else 3.0, sigma=1.7)


def _bessel(layer, net, d):
    u = d * float(np.float32(1 / layer.cutoff))
    freq = net.w(layer.frequencies)
    return dref.envelope(u, layer.envelope_exponent)[:, None] * torch.sin(freq[None, :] * u[:, None])


def _angles(v, pairs, second_scale, dtype):
    """theta (T,) between ``v[n]`` and ``second_scale * v[m]``; a self pair (n == m, second_scale -1) is the constant
    pi."""
    theta = torch.full((int(pairs.shape[0]),), math.pi if second_scale < 0 else 0.0, dtype=dtype)
    real = torch.nonzero(pairs[:, 0] != pairs[:, 1])[:, 0]
    if len(real):
        p = pairs[real]
        theta = theta.index_put((real,), dref.vector_angle(v[p[:, 0]], second_scale * v[p[:, 1]]))
    return theta


def _layers_of(model, name):
    return [layer for layer in model.layers if type(layer).__name__ == name]


def mxmnet_forward(weights, b, model, xyz=None, dtype=torch.float64):
    """Model output of MXMNet on a synth.mxmnet_batch ``b``: ``(G, L)`` for ``output_embedding="graph"``;
    ``weights``: arrays in ``model.weights`` order; ``xyz``: coordinates tensor (defaults to the batch's)."""
    cfg = model.config
    net = _Net(weights_of(model, weights), dtype)
    ei, ri, a1, a2 = (torch.from_numpy(x) for x in flat_indices(b))
    if xyz is None:
        xyz = torch.tensor(b["node_coordinates"], dtype=dtype)
    emb = _layers_of(model, "EmbeddingDimeBlock")
    if emb:
        n = net.w(emb[0].embeddings)[torch.from_numpy(np.asarray(b["node_number"])).long()]
    else:
        n = torch.tensor(b["node_attributes"], dtype=dtype)
    mlps = _layers_of(model, "MLP")   # GraphMLP is MLP: rbf_l, sbf_1, sbf_2, rbf_g [, output]
    if cfg["output_embedding"] == "node":
        return net.mlp(mlps[0], n) if mlps else n

    bessel_l, bessel_g = _layers_of(model, "BesselBasisLayer")
    sbf_layer_1, sbf_layer_2 = _layers_of(model, "SphericalBasisLayer")
    v = xyz[ei[:, 0]] - xyz[ei[:, 1]]
    d = torch.linalg.norm(v, dim=-1)
    rbf_l = _bessel(bessel_l, net, d)
    sbf_1 = dref.spherical_basis(d, _angles(v, a1, 1.0, dtype), a1[:, 1], sbf_layer_1, dtype)
    sbf_2 = dref.spherical_basis(d, _angles(v, a2, -1.0, dtype), a2[:, 1], sbf_layer_2, dtype)
    d_g = torch.linalg.norm(xyz[ri[:, 0]] - xyz[ri[:, 1]], dim=-1)
    rbf_g = _bessel(bessel_g, net, d_g)

    if cfg["use_edge_attributes"]:
        embed_e = _layers_of(model, "OptionalInputEmbedding")[0]
        if embed_e.use_embedding:
            ed = net.w(embed_e.embeddings)[torch.from_numpy(np.asarray(b["edge_number"])).long()]
        else:
            ed = torch.tensor(b["edge_weights"], dtype=dtype)
        rbf_l = torch.cat([rbf_l, ed], dim=-1)

    rbf_l, sbf_1, sbf_2, rbf_g = (net.mlp(m, x) for m, x in zip(mlps[:4], (rbf_l, sbf_1, sbf_2, rbf_g)))
    h, outs = n, []
    for glob, loc in zip(model.global_blocks, model.local_blocks):
        h = net.global_mp(glob, h, rbf_g, ri)
        h, t = net.local_mp(loc, h, rbf_l, sbf_1, sbf_2, ei, a1, a2)
        outs.append(t)
    out = outs[0]
    for t in outs[1:]:
        out = out + t
    ns = b["node_splits"]
    graph = torch.from_numpy(np.repeat(np.arange(len(ns) - 1), np.diff(ns)))
    out = net.pool(out, graph, len(ns) - 1, cfg["node_pooling_args"].get("pooling_method", "mean"))
    if cfg["use_output_mlp"]:
        out = net.mlp(mlps[4], out)
    return out


def energy_forces(weights, b, model, dtype=torch.float64):
    """(E (G, 1), F = -dE/dx (N, 3)) of the restatement."""
    xyz = torch.tensor(b["node_coordinates"], dtype=dtype, requires_grad=True)
    e = mxmnet_forward(weights, b, model, xyz=xyz, dtype=dtype)
    (g,) = torch.autograd.grad(e.sum(), xyz)
    return e.detach(), -g
