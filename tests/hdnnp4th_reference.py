"""Differentiable torch-CPU restatement of HDNNP4th (float64 / float32), written from the formulas of the charge
equilibration as kgcnn states them (hdnnp_conv.py docstrings, Ko et al. 2021), not from the reference code:

* per molecule, A_ii = J[z_i] + 1 / (sigma_i sqrt(pi)), A_ij = erf(r_ij / (sqrt(2) gamma_ij)) / r_ij over all atom pairs,
  gamma_ij = sqrt(sigma_i^2 + sigma_j^2); [[A, 1], [1^T, 0]] [Q; lambda] = [chi; Qtot] by ``torch.linalg.solve``;
* E_elec = sum over range_indices of q_i q_j f_ij / multiplicity + sum_i q_i^2 / (2 sqrt(pi) sigma_i);
* E_qmmm = sum_i q_i esp_i;
* the model: rep = [G2, G4], rep_esp = [rep, esp], chi = MLP_charge(rep_esp) + esp, (q, E_elec) = CENT, E = sum
  MLP_local([rep_esp, q]) + E_elec + E_qmmm; forces with the esp chain dE/dx + dE/desp * desp/dx.

G2, G4 and the relational MLP come from tests/hdnnp_reference.py.  Indices are global (already shifted into the batch)."""
import math

import numpy as np
import torch

import hdnnp_reference as ref2


def _pair_f(r, gamma):
    return torch.erf(r / (math.sqrt(2.0) * gamma)) / r


def cent_molecule(z, xyz, chi, qtot, sigma_tab, j_tab):
    """Charges (n,) of one molecule: z (n,) numpy, xyz (n, 3), chi (n,), qtot scalar tensor."""
    dt = xyz.dtype
    n = xyz.shape[0]
    sig = torch.as_tensor(np.asarray(sigma_tab), dtype=dt)[torch.as_tensor(z)]
    jj = torch.as_tensor(np.asarray(j_tab), dtype=dt)[torch.as_tensor(z)]
    a = torch.diag(jj + 1.0 / sig / math.sqrt(math.pi))
    if n > 1:
        i, j = torch.triu_indices(n, n, offset=1)
        r = torch.linalg.norm(xyz[i] - xyz[j], dim=-1)
        f = _pair_f(r, torch.sqrt(sig[i] ** 2 + sig[j] ** 2))
        off = torch.zeros((n, n), dtype=dt).index_put((i, j), f)
        a = a + off + off.T
    m = torch.zeros((n + 1, n + 1), dtype=dt)
    m = m + torch.nn.functional.pad(a, (0, 1, 0, 1))
    border = torch.zeros((n + 1, n + 1), dtype=dt)
    border[:n, n] = 1.0
    border[n, :n] = 1.0
    m = m + border
    rhs = torch.cat([chi.reshape(n), qtot.reshape(1).to(dt)])
    return torch.linalg.solve(m, rhs)[:n]


def cent(z, xyz, chi, qtot, node_splits, sigma_tab, j_tab):
    """Flat charges (N,) of a batch."""
    out = []
    for g in range(len(node_splits) - 1):
        lo, hi = int(node_splits[g]), int(node_splits[g + 1])
        if hi > lo:
            out.append(cent_molecule(z[lo:hi], xyz[lo:hi], chi[lo:hi], qtot[g], sigma_tab, j_tab))
    return torch.cat(out) if out else torch.zeros(0, dtype=xyz.dtype)


def _graph_of(node_splits):
    return torch.as_tensor(np.repeat(np.arange(len(node_splits) - 1), np.diff(node_splits)))


def gauss_energy(z, xyz, q, ij, node_splits, sigma_tab, multiplicity=2.0):
    """(G, 1): pair term over the global index pairs ij (M, 2), self term over the atoms."""
    dt = xyz.dtype
    g_count = len(node_splits) - 1
    sig = torch.as_tensor(np.asarray(sigma_tab), dtype=dt)[torch.as_tensor(z)]
    q = q.reshape(-1)
    i, j = torch.as_tensor(ij[:, 0]), torch.as_tensor(ij[:, 1])
    r = torch.linalg.norm(xyz[i] - xyz[j], dim=-1)
    pair = q[i] * q[j] * _pair_f(r, torch.sqrt(sig[i] ** 2 + sig[j] ** 2))
    graph = _graph_of(node_splits)
    e_pair = torch.zeros(g_count, dtype=dt).index_add(0, graph[i], pair)
    if multiplicity:
        e_pair = e_pair / multiplicity
    self_e = torch.where(sig != 0, q * q / torch.where(sig != 0, sig, torch.ones_like(sig)), torch.zeros_like(q))
    e_self = torch.zeros(g_count, dtype=dt).index_add(0, graph, self_e / (2.0 * math.sqrt(math.pi)))
    return (e_pair + e_self).reshape(-1, 1)


def qmmm_energy(q, esp, node_splits):
    return torch.zeros(len(node_splits) - 1, dtype=q.dtype).index_add(
        0, _graph_of(node_splits), q.reshape(-1) * esp.reshape(-1)).reshape(-1, 1)


def model_outputs(model, weights, b, dt, xyz=None, esp=None):
    """Every output of a ``HDNNP4th.make_model_behler`` model in fork configuration: dict with ``charge`` (N,),
    ``electrostatic_energy`` (G, 1), ``qmmm`` (G, 1) and ``energy`` (G, 1).  ``weights``: the charge MLP's then the
    local MLP's (kernel, bias) per layer; ``b`` a synth.hdnnp4th_batch with global ``ij`` / ``ijk``."""
    x = torch.as_tensor(b["node_coordinates"], dtype=dt) if xyz is None else xyz
    e_in = torch.as_tensor(b["esp"], dtype=dt) if esp is None else esp
    z, ns = b["node_number"], b["node_splits"]
    cent_layer = next(lay for lay in model.layers if type(lay).__name__ == "CENTChargePlusElectrostaticEnergy")
    mlps =[lay for lay in model.layers if type(lay).__name__ == "RelationalMLP"]
    rep = ref2.representation(model, z, x, b["ij"], b["ijk"])
    rep_esp = torch.cat([rep, e_in.reshape(-1, 1)], dim=-1)
    ws = list(weights)
    h = rep_esp
    for li in range(mlps[0]._depth):
        h = ref2.relational_dense(h, ws[2 * li], ws[2 * li + 1], z, mlps[0]._conf_activation[li])
    chi = h.reshape(-1) + e_in.reshape(-1)
    qt = torch.as_tensor(b["total_charge"], dtype=dt).reshape(-1)
    q = cent(z, x, chi, qt, ns, cent_layer.weight_sigma, cent_layer.weight_j)
    mult = cent_layer.multiplicity
    e_elec = gauss_energy(z, x, q, b["ij"], ns, cent_layer.weight_sigma, mult)
    out = {"charge": q, "electrostatic_energy": e_elec, "chi": chi}
    if len(mlps) > 1:
        off = 2 * mlps[0]._depth
        h = torch.cat([rep_esp, q.reshape(-1, 1)], dim=-1)
        for li in range(mlps[1]._depth):
            h = ref2.relational_dense(h, ws[off + 2 * li], ws[off + 2 * li + 1], z, mlps[1]._conf_activation[li])
        e_short = torch.zeros((len(ns) - 1, 1), dtype=dt).index_add(0, _graph_of(ns), h)
        e_qmmm = qmmm_energy(q, e_in, ns)
        out.update({"qmmm": e_qmmm, "energy": e_short + e_elec + e_qmmm})
    return out


def forces(model, weights, b, dt):
    """dE/dx + dE/desp * desp/dx (N, 3) of the total energy, through autograd (is_physical_force=False)."""
    x = torch.as_tensor(b["node_coordinates"], dtype=dt).requires_grad_(True)
    e = torch.as_tensor(b["esp"], dtype=dt).requires_grad_(True)
    out = model_outputs(model, weights, b, dt, xyz=x, esp=e)
    gx, ge = torch.autograd.grad(out["energy"].sum(), [x, e])
    return gx + ge.reshape(-1, 1) * torch.as_tensor(b["esp_grad"], dtype=dt)


def padded(values, node_splits):
    """(G, Nmax) zero-padded rows of a flat per-atom vector (one row per molecule)."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    ns = np.asarray(node_splits)
    counts = np.diff(ns)
    out = np.zeros((len(counts), int(counts.max()) if counts.size else 0))
    for g in range(len(counts)):
        out[g, :counts[g]] = v[ns[g]:ns[g + 1]]
    return out
