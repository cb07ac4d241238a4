"""Differentiable torch-CPU restatement of HDNNP2nd (float64 / float32), written from the formulas of Behler's symmetry
functions as kgcnn states them (acsf_conv.py docstrings), not from the reference code:

* G2_i[rel(z_j), m] += exp(-eta_m (r_ij - rs_m)^2) fc_m(r_ij)
* G4_i[rel(z_j, z_k), m] += 2^(1-zeta_m) (1 + lambda_m cos_ijk)^zeta_m exp(-eta_m (r_ij^2 + r_ik^2 + r_jk^2))
  fc_m(r_ij) fc_m(r_ik) fc_m(r_jk) / multiplicity,   cos_ijk = (x_i - x_j).(x_i - x_k) / r_ij / r_ik
* fc(r) = 0.5 (cos(pi clip(r, -rc, rc) / rc) + 1); an unmapped element contributes nothing
* RelationalMLP: x <- act(x W_l[z] + b_l) per layer; energy = per-molecule sum of the last layer.

Indices are global (already shifted into the batch)."""
import math

import numpy as np
import torch


def _fc(r, rc):
    return 0.5 * (torch.cos(math.pi * torch.maximum(torch.minimum(r, rc), -rc) / rc) + 1.0)


def g2(z, xyz, ij, table, rmap, nrel, ncenter=0):
    """table (nrel, m, 3) or (ncenter, nrel, m, 3) numpy; rmap: dict z -> slot.  Returns (N, nrel*m)."""
    dt = xyz.dtype
    tab = torch.as_tensor(np.asarray(table), dtype=dt)
    m = tab.shape[-2]
    n = xyz.shape[0]
    slot = np.array([rmap.get(int(v), -1) for v in z])
    i, j = ij[:, 0], ij[:, 1]
    sj = slot[j]
    keep = sj >= 0
    if ncenter:
        keep &= slot[i] >= 0
    i, j, sj = i[keep], j[keep], sj[keep]
    p = tab[slot[i], sj] if ncenter else tab[sj]                   # (M, m, 3)
    r = torch.linalg.norm(xyz[i] - xyz[j], dim=-1, keepdim=True)   # (M, 1)
    eta, rs, rc = p[..., 0], p[..., 1], p[..., 2]
    val = torch.exp(-eta * (r - rs) ** 2) * _fc(r, rc)
    out = torch.zeros((n, nrel, m), dtype=dt)
    out = out.index_put((torch.as_tensor(i), torch.as_tensor(sj)), val, accumulate=True)
    return out.reshape(n, nrel * m)


def g4(z, xyz, ijk, table, rmap, pmap, nrel, multiplicity=None, ncenter=0):
    """table (nrel, m, 4) or (ncenter, nrel, m, 4); pmap: dict (z_j, z_k) -> relation."""
    dt = xyz.dtype
    tab = torch.as_tensor(np.asarray(table), dtype=dt)
    m = tab.shape[-2]
    n = xyz.shape[0]
    i, j, k = ijk[:, 0], ijk[:, 1], ijk[:, 2]
    rel = np.array([pmap.get((int(z[a]), int(z[b])), -1) for a, b in zip(j, k)], dtype=np.int64)
    keep = rel >= 0
    slot = np.array([rmap.get(int(v), -1) for v in z])
    if ncenter:
        keep &= slot[i] >= 0
    i, j, k, rel = i[keep], j[keep], k[keep], rel[keep]
    p = tab[slot[i], rel] if ncenter else tab[rel]
    vij, vik, vjk = xyz[i] - xyz[j], xyz[i] - xyz[k], xyz[j] - xyz[k]
    rij = torch.linalg.norm(vij, dim=-1, keepdim=True)
    rik = torch.linalg.norm(vik, dim=-1, keepdim=True)
    rjk = torch.linalg.norm(vjk, dim=-1, keepdim=True)
    cos = (vij * vik).sum(-1, keepdim=True) / rij / rik
    eta, zeta, lam, rc = p[..., 0], p[..., 1], p[..., 2], p[..., 3]
    ang = torch.pow(2.0 * torch.ones_like(zeta), 1.0 - zeta) * torch.pow(1.0 + lam * cos, zeta)
    if multiplicity is not None:
        ang = ang / multiplicity
    val = ang * torch.exp(-eta * (rij ** 2 + rik ** 2 + rjk ** 2)) * _fc(rij, rc) * _fc(rik, rc) * _fc(rjk, rc)
    out = torch.zeros((n, nrel, m), dtype=dt)
    out = out.index_put((torch.as_tensor(i), torch.as_tensor(rel)), val, accumulate=True)
    return out.reshape(n, nrel * m)


ACTS = {"tanh": torch.tanh, "linear": lambda v: v, "swish": lambda v: v * torch.sigmoid(v)}


def relational_dense(x, kernel, bias, rel, act="linear"):
    """act(x W[rel] + b); a relation outside the table uses a zero kernel."""
    nrel = kernel.shape[0]
    rel = torch.as_tensor(np.asarray(rel), dtype=torch.int64)
    ok = (rel >= 0) & (rel < nrel)
    w = kernel[torch.where(ok, rel, torch.zeros_like(rel))] * ok.to(kernel.dtype)[:, None, None]
    y = torch.einsum("nk,nku->nu", x, w)
    if bias is not None:
        y = y + bias
    return ACTS[act](y)


def tables(layer):
    """(table, rmap dict, pmap dict) of an engine ACSF layer (numpy side only)."""
    rmap = {int(zz): int(s) for zz, s in enumerate(layer.reverse_mapping) if 0 <= s < 2 ** 31 - 1}
    pmap = {}
    if hasattr(layer, "reverse_pair_mapping"):
        rp = layer.reverse_pair_mapping
        for a in range(rp.shape[0]):
            for b in range(rp.shape[1]):
                if 0 <= rp[a, b] < 2 ** 31 - 1:
                    pmap[(a, b)] = int(rp[a, b])
    return layer._param_table, rmap, pmap


def representation(model, z, xyz, ij, ijk):
    g2l, g4l = model.layers[0], model.layers[1]
    t2, r2, _ = tables(g2l)
    t4, r4, p4 = tables(g4l)
    a = g2(z, xyz, ij, t2, r2, g2l.num_relations, g2l.num_centers)
    b = g4(z, xyz, ijk, t4, r4, p4, g4l.num_relations, g4l.multiplicity, g4l.num_centers)
    return torch.cat([a, b], dim=-1)


def energy(model, weights, z, xyz, ij, ijk, node_splits):
    """Per-molecule energy (G, 1) of a ``make_model_behler`` model with weights {name: tensor} in ``model.weights``
    order (kernel, bias per layer)."""
    x = representation(model, z, xyz, ij, ijk)
    mlp = model.layers[3]
    ws = list(weights)
    for li in range(mlp._depth):
        x = relational_dense(x, ws[2 * li], ws[2 * li + 1], z, mlp._conf_activation[li])
    seg = torch.as_tensor(np.repeat(np.arange(len(node_splits) - 1), np.diff(node_splits)))
    out = torch.zeros((len(node_splits) - 1, x.shape[-1]), dtype=x.dtype)
    return out.index_add(0, seg, x)
