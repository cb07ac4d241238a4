"""HDNNP4th on the engine (the fork's force_hdnnp4th.py / charge_hdnnp4th.py): the charge-equilibration solve and the
Gaussian-charge electrostatics (csrc/mp_cent.hip) and their reverse against a torch restatement
(tests/hdnnp4th_reference.py), the fork's model for every output embedding, forces with the esp chain, determinism and
graph replay, training of the charge and total-energy models, and the guard on force training."""
import numpy as np
import pytest
import torch

import hdnnp4th_reference as ref
from gcnn_keras_amd import _ffi, synth
from gcnn_keras_amd.layers.conv.hdnnp_conv import (CENTCharge, CENTChargePlusElectrostaticEnergy,
                                                   ElectrostaticEnergyGaussCharge)
from gcnn_keras_amd.literature import HDNNP4th
from gcnn_keras_amd.model.force import EnergyForceModel
from gcnn_keras_amd.ragged import RaggedTensor
from parity import assert_forces_close, assert_rows_close

pytestmark = pytest.mark.gpu

# A kernel gradient sums the rows of ~1000 atoms of one element (tests/test_gpu_hdnnp.py): 4e-5 per row.
GRAD_RTOL = 4e-5


def _rag(values, splits):
    return RaggedTensor.from_numpy(values, splits)


def _global(idx, idx_splits, node_splits):
    shift = np.repeat(node_splits[:-1], np.diff(idx_splits))
    return idx + shift[:, None]


def _batch(num_graphs=6, seed=5, mixed=False, angles=None):
    b = synth.hdnnp4th_batch(num_graphs=num_graphs, seed=seed, mixed=mixed, angles=angles)
    b["ij"] = _global(b["edge_indices"], b["edge_splits"], b["node_splits"])
    b["ijk"] = _global(b["angle_indices"], b["angle_splits"], b["node_splits"])
    return b


def _inputs(b, esp_scale=1.0):
    return [_rag(b["node_number"], b["node_splits"]), _rag(b["node_coordinates"], b["node_splits"]),
            _rag(b["edge_indices"], b["edge_splits"]), _rag(b["angle_indices"], b["angle_splits"]),
            torch.as_tensor(b["total_charge"]).cuda(), _rag(b["esp"] * np.float32(esp_scale), b["node_splits"]),
            _rag(b["esp_grad"] * np.float32(esp_scale), b["node_splits"])]


def _chi(b, seed=3):
    return (np.random.default_rng(seed).normal(size=len(b["node_number"])) * 0.3).astype(np.float32)


def _engine_charges(layer, b, chi, xyz=None, chi_t=None):
    z = _rag(b["node_number"], b["node_splits"])
    x = _rag(b["node_coordinates"], b["node_splits"]) if xyz is None else xyz
    c = _rag(chi.reshape(-1, 1), b["node_splits"]) if chi_t is None else chi_t
    return layer([z, c, x, torch.as_tensor(b["total_charge"]).cuda()])


def _ref_charges(layer, b, chi, dt, xyz=None, chi_t=None):
    x = torch.as_tensor(b["node_coordinates"], dtype=dt) if xyz is None else xyz
    c = torch.as_tensor(chi, dtype=dt) if chi_t is None else chi_t
    return ref.cent(b["node_number"], x, c, torch.as_tensor(b["total_charge"], dtype=dt).reshape(-1),
                    b["node_splits"], layer.weight_sigma, layer.weight_j)


# ------------------------------------------------------------------------------------------- 1. the charge solve
@pytest.mark.parametrize("mixed", [False, True])
def test_charge_solve_per_molecule(mixed):
    b = _batch(num_graphs=10 if mixed else 128, seed=11, mixed=mixed)
    layer = CENTCharge()
    chi = _chi(b)
    q = _engine_charges(layer, b, chi).values.cpu().numpy().reshape(-1)
    ns = b["node_splits"]
    r32, r64 = (ref.padded(_ref_charges(layer, b, chi, dt).numpy(), ns) for dt in (torch.float32, torch.float64))
    # a charge is measured against its molecule's largest charge (one row per molecule): a near-zero charge carries
    # the solve's absolute rounding, whoever computes it
    assert_rows_close(ref.padded(q, ns), r32, r64, what="CENT charges (mixed=%s)" % mixed)
    qt = b["total_charge"].reshape(-1)
    for g in range(len(ns) - 1):
        qg = q[ns[g]:ns[g + 1]].astype(np.float64)
        assert abs(qg.sum() - qt[g]) <= 1e-5 * max(1.0, np.abs(qg).sum()), g
    if mixed:
        sig = layer.weight_sigma.astype(np.float64)
        jj = layer.weight_j.astype(np.float64)
        z, x = b["node_number"], b["node_coordinates"].astype(np.float64)
        for g in range(len(ns) - 1):
            lo, n = ns[g], ns[g + 1] - ns[g]
            if n == 1:
                assert abs(q[lo] - qt[g]) <= 1e-6
            if n == 2:
                a = jj[z[lo]] + 1.0 / sig[z[lo]] / np.sqrt(np.pi)
                bb = jj[z[lo + 1]] + 1.0 / sig[z[lo + 1]] / np.sqrt(np.pi)
                r = np.linalg.norm(x[lo] - x[lo + 1])
                from math import erf
                f = erf(r / (np.sqrt(2.0) * np.sqrt(sig[z[lo]] ** 2 + sig[z[lo + 1]] ** 2))) / r
                q1 = (float(chi[lo]) - float(chi[lo + 1]) + (bb - f) * qt[g]) / (a + bb - 2.0 * f)
                assert abs(q[lo] - q1) <= 1e-6 * max(1.0, abs(q1)) and abs(q[lo + 1] - (qt[g] - q1)) <= 1e-6 * max(
                    1.0, abs(q1))


def test_molecule_above_the_bound_raises():
    n = _ffi.MP_CENT_MAX_ATOMS + 1
    rng = np.random.default_rng(0)
    b = {"node_number": np.ones(n, np.int64), "node_coordinates": rng.normal(size=(n, 3)).astype(np.float32) * 10,
         "node_splits": np.array([0, n], np.int64), "total_charge": np.zeros((1, 1), np.float32)}
    with pytest.raises(ValueError, match=str(_ffi.MP_CENT_MAX_ATOMS)):
        _engine_charges(CENTCharge(), b, np.zeros(n, np.float32))


# ------------------------------------------------------------------------------------------- 2. the solve's reverse
@pytest.mark.parametrize("mixed", [False, True])
def test_charge_solve_reverse(mixed):
    b = _batch(num_graphs=10 if mixed else 8, seed=13, mixed=mixed)
    layer = CENTCharge()
    chi = _chi(b, 4)
    n = len(b["node_number"])
    gq = torch.randn(n, 1, generator=torch.Generator().manual_seed(5))
    xd = torch.as_tensor(b["node_coordinates"]).cuda().requires_grad_(True)
    cd = torch.as_tensor(chi.reshape(-1, 1)).cuda().requires_grad_(True)
    ns_t = torch.as_tensor(b["node_splits"]).cuda()
    q = _engine_charges(layer, b, chi, xyz=RaggedTensor(xd, ns_t), chi_t=RaggedTensor(cd, ns_t)).values
    chi_bar, x_bar = torch.autograd.grad(q, [cd, xd], grad_outputs=gq.cuda())
    refs = []
    for dt in (torch.float32, torch.float64):
        x = torch.as_tensor(b["node_coordinates"], dtype=dt).requires_grad_(True)
        c = torch.as_tensor(chi, dtype=dt).requires_grad_(True)
        qr = _ref_charges(layer, b, chi, dt, xyz=x, chi_t=c)
        gc, gx = torch.autograd.grad(qr, [c, x], grad_outputs=gq.reshape(-1).to(dt))
        refs.append((gc.numpy(), gx.numpy()))
    ns = b["node_splits"]
    assert_rows_close(ref.padded(chi_bar.cpu().numpy(), ns), ref.padded(refs[0][0], ns), ref.padded(refs[1][0], ns),
                      what="CENT chi_bar")
    assert_forces_close(x_bar.cpu().numpy(), refs[0][1], refs[1][1], ns, what="CENT x_bar")


# ------------------------------------------------------------------------------------------- 3. electrostatic energy
@pytest.mark.parametrize("which,multiplicity", [("standalone", 2.0), ("standalone", None), ("combined", 2.0),
                                                ("combined", None)])
def test_gauss_energy_and_reverse(which, multiplicity):
    b = _batch(num_graphs=10, seed=17, mixed=True)
    ns = b["node_splits"]
    n = len(b["node_number"])
    qv = (np.random.default_rng(6).normal(size=n) * 0.4).astype(np.float32)
    layer = ElectrostaticEnergyGaussCharge(multiplicity=multiplicity) if which == "standalone" else \
        CENTChargePlusElectrostaticEnergy(multiplicity=multiplicity)
    xd = torch.as_tensor(b["node_coordinates"]).cuda().requires_grad_(True)
    qd = torch.as_tensor(qv.reshape(-1, 1)).cuda().requires_grad_(True)
    ns_t = torch.as_tensor(ns).cuda()
    from gcnn_keras_amd.layers.conv.hdnnp_conv import gauss_energy
    e = gauss_energy(layer, _rag(b["node_number"], ns), RaggedTensor(qd, ns_t), RaggedTensor(xd, ns_t),
                     _rag(b["edge_indices"], b["edge_splits"]))
    ge = torch.randn(len(ns) - 1, 1, generator=torch.Generator().manual_seed(7))
    q_bar, x_bar = torch.autograd.grad(e, [qd, xd], grad_outputs=ge.cuda())
    refs = []
    for dt in (torch.float32, torch.float64):
        x = torch.as_tensor(b["node_coordinates"], dtype=dt).requires_grad_(True)
        q = torch.as_tensor(qv, dtype=dt).requires_grad_(True)
        er = ref.gauss_energy(b["node_number"], x, q, b["ij"], ns, layer.weight_sigma, multiplicity)
        gq, gx = torch.autograd.grad(er, [q, x], grad_outputs=ge.to(dt))
        refs.append((er.detach().numpy(), gq.numpy(), gx.numpy()))
    what = "%s mult=%s" % (which, multiplicity)
    assert_rows_close(e.detach().cpu().numpy(), refs[0][0], refs[1][0], what="E_elec " + what)
    assert_rows_close(ref.padded(q_bar.cpu().numpy(), ns), ref.padded(refs[0][1], ns), ref.padded(refs[1][1], ns),
                      what="q_bar " + what)
    assert_forces_close(x_bar.cpu().numpy(), refs[0][2], refs[1][2], ns, what="x_bar " + what)


def test_combined_layer_uses_the_bohr_table():
    combined, standalone = CENTChargePlusElectrostaticEnergy(), ElectrostaticEnergyGaussCharge()
    assert np.array_equal(combined.weight_sigma, CENTCharge().weight_sigma)
    assert not np.array_equal(combined.weight_sigma, standalone.weight_sigma)


# ------------------------------------------------------------------------------------------- 4. the fork's model
def _model(embedding="charge+qm_energy", seed=12):
    model = HDNNP4th.make_model_behler(**synth.hdnnp4th_model_kwargs(output_embedding=embedding))
    p = list(synth.hdnnp4th_params(seed=seed).values())
    model.set_weights(p[:len(model.weights)])
    return model, p


def _ref_out(model, p, b, dt, **kw):
    return ref.model_outputs(model, [torch.as_tensor(v, dtype=dt) for v in p], b, dt, **kw)


@pytest.mark.parametrize("embedding", ["graph", "total_energy", "charge", "electrostatic_energy", "charge+qm_energy"])
def test_fork_model_every_output_embedding(embedding):
    b = _batch(num_graphs=6, seed=31)
    model, p = _model(embedding)
    out = model(_inputs(b))
    r = [_ref_out(model, p, b, dt) for dt in (torch.float32, torch.float64)]
    ns = b["node_splits"]
    charge_refs = [ref.padded(x["charge"].detach().numpy(), ns) for x in r]
    if embedding in ("graph", "total_energy"):
        assert_rows_close(out.cpu().numpy(), r[0]["energy"].detach().numpy(), r[1]["energy"].detach().numpy(),
                          what="HDNNP4th energy")
    elif embedding == "charge":
        assert tuple(out.shape) == (6, 22, 1)
        assert_rows_close(out.cpu().numpy()[..., 0], *charge_refs, what="HDNNP4th charge")
    elif embedding == "electrostatic_energy":
        assert_rows_close(out.cpu().numpy(), r[0]["electrostatic_energy"].detach().numpy(),
                          r[1]["electrostatic_energy"].detach().numpy(), what="HDNNP4th E_elec")
    else:
        charge, energy = out
        assert_rows_close(charge.cpu().numpy()[..., 0], *charge_refs, what="HDNNP4th charge")
        assert_rows_close(energy.cpu().numpy(), r[0]["energy"].detach().numpy(), r[1]["energy"].detach().numpy(),
                          what="HDNNP4th energy")


# ------------------------------------------------------------------------------------------- 5. forces
def _efm(model, esp=True):
    kw = {"esp_input": 5, "esp_grad_input": 6} if esp else {}
    return EnergyForceModel(model_energy=model, energy_output=1, is_physical_force=False, output_squeeze_states=True,
                            output_as_dict=False, **kw)


def test_fork_forces_with_esp_chain():
    b = _batch(num_graphs=6, seed=41)
    model, p = _model()
    charge, energy, force = _efm(model)(_inputs(b))
    assert tuple(charge.shape) == (6, 22, 1) and tuple(energy.shape) == (6, 1)
    refs = [ref.forces(model, [torch.as_tensor(v, dtype=dt) for v in p], b, dt).numpy()
            for dt in (torch.float32, torch.float64)]
    f = force.cpu().numpy().reshape(-1, 3)       # padded (6, 22, 3): every molecule has 22 atoms
    assert_forces_close(f, refs[0], refs[1], b["node_splits"], what="HDNNP4th forces")
    # without an external field the forces of every molecule sum to zero (translation invariance)
    b0 = dict(b, esp=np.zeros_like(b["esp"]), esp_grad=np.zeros_like(b["esp_grad"]))
    _, _, f0 = _efm(model)(_inputs(b0))
    f0 = f0.cpu().numpy().reshape(-1, 22, 3).astype(np.float64)
    scale = np.abs(f0).max(axis=(1, 2))
    assert np.all(np.abs(f0.sum(axis=1)).max(axis=1) <= 1e-5 * 22 * scale)


# ------------------------------------------------------------------------------------------- 6. determinism, replay
def test_deterministic_runs_streams_and_replay():
    b = _batch(num_graphs=8, seed=51)
    model, _ = _model()
    efm = _efm(model)
    inputs = _inputs(b)

    def run():
        c, e, f = efm(inputs)
        torch.cuda.synchronize()
        return [t.detach().cpu() for t in (c, e, f)]

    a = run()
    bb = run()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c = run()
    torch.cuda.synchronize()
    for u, v, w in zip(a, bb, c):
        assert torch.equal(u, v) and torch.equal(u, w)
    eager = model(inputs)
    second = model(inputs)
    third = model(inputs)
    assert model.last_route == "graph"
    for u, v, w in zip(eager, second, third):
        assert torch.equal(u, v) and torch.equal(u, w)
    assert torch.equal(eager[0].cpu(), a[0]) and torch.equal(eager[1].cpu(), a[1])


# ------------------------------------------------------------------------------------------- 7. charge-model training
def _charge_target(b, seed):
    t = (np.random.default_rng(seed).normal(size=(len(b["node_number"]), 1)) * 0.3).astype(np.float32)
    return t, RaggedTensor.from_numpy(t, b["node_splits"])


# The charge network's last bias shifts chi by the same amount on every atom; the constraint sum Q = Qtot absorbs that
# shift into lambda, so no charge depends on it: its gradient is zero in exact arithmetic (1^T w = 0 per molecule) and
# only rounding is left to compare.  It is held to zero against the scale of the other gradients instead.
CHARGE_LAST_BIAS = 3


def _check_weight_grads(model, grads, refs32, refs64):
    scale = max(float(np.abs(g.cpu().numpy()).max()) for g in grads)
    for k, ((name, _), gg, r32, r64) in enumerate(zip(model.weights, grads, refs32, refs64)):
        if k == CHARGE_LAST_BIAS:
            assert float(np.abs(gg.cpu().numpy()).max()) <= 1e-6 * scale and float(np.abs(r64).max()) <= 1e-12 * scale
            continue
        width = gg.shape[-1]
        assert_rows_close(gg.cpu().numpy().reshape(-1, width), r32.reshape(-1, width), r64.reshape(-1, width),
                          what="dLoss/d" + name, rtol=GRAD_RTOL)


def _ref_charge_loss(model, ws, b, t, dt):
    q = ref.model_outputs(model, ws, b, dt)["charge"]
    return ((q - torch.as_tensor(t.reshape(-1), dtype=dt)) ** 2).mean()


def test_charge_model_gradients_and_sgd_track_float64():
    b = _batch(num_graphs=4, seed=61, mixed=True, angles=True)     # 1, 2, 3 and 22 atoms: ragged vs padded
    model, p = _model("charge")
    t_np, target = _charge_target(b, 1)
    inputs = _inputs(b)
    for w in model.trainable_weights:
        w.requires_grad_(True)
    from gcnn_keras_amd.model.losses import mean_squared_error
    loss = mean_squared_error(model(inputs), target)
    grads = torch.autograd.grad(loss, model.trainable_weights)
    model.requires_grad_(False)
    refs = []
    for dt in (torch.float32, torch.float64):
        ws = [torch.as_tensor(v, dtype=dt).requires_grad_(True) for v in p[:4]]
        refs.append([g.numpy() for g in torch.autograd.grad(_ref_charge_loss(model, ws, b, t_np, dt), ws)])
    _check_weight_grads(model, grads, refs[0], refs[1])
    lr = 0.05
    model.compile(optimizer=torch.optim.SGD(model.trainable_weights, lr=lr), loss="mean_squared_error")
    got = [model.train_on_batch(inputs, target) for _ in range(3)]
    ws = [torch.as_tensor(v, dtype=torch.float64).requires_grad_(True) for v in p[:4]]
    want = []
    for _ in range(3):
        lo = _ref_charge_loss(model, ws, b, t_np, torch.float64)
        want.append(float(lo.detach()))
        gs = torch.autograd.grad(lo, ws)
        with torch.no_grad():
            for w_, g_ in zip(ws, gs):
                w_ -= lr * g_
    assert np.allclose(got, want, rtol=1e-4), (got, want)
    for k, ((name, tw), w64, w0) in enumerate(zip(model.weights, ws, p[:4])):
        moved = w64.detach().numpy() - w0
        diff = tw.detach().cpu().numpy() - w64.detach().numpy()
        if k == CHARGE_LAST_BIAS:       # does not move in exact arithmetic
            assert np.abs(diff).max() <= 1e-6, name
            continue
        assert np.abs(diff).max() <= 1e-3 * max(np.abs(moved).max(), 1e-12), name


def test_charge_model_adam_clipnorm_lowers_loss_and_is_deterministic():
    b = _batch(num_graphs=4, seed=71, mixed=True, angles=True)
    _, target = _charge_target(b, 2)
    runs = []
    for _ in range(2):
        model, _ = _model("charge")
        model.compile(optimizer="adam", loss="mean_squared_error", clipnorm=1.0)
        inputs = _inputs(b)
        losses = [model.train_on_batch(inputs, target) for _ in range(5)]
        runs.append((losses, [t.detach().cpu().clone() for t in model.trainable_weights]))
    assert runs[0][0][-1] < runs[0][0][0]
    assert runs[0][0] == runs[1][0]
    for u, v in zip(runs[0][1], runs[1][1]):
        assert torch.equal(u, v)


# ------------------------------------------------------------------------------------------- 8. total-energy training
def test_total_energy_model_gradients_and_adam_step():
    b = _batch(num_graphs=4, seed=81)
    model, p = _model("graph")
    inputs = _inputs(b)
    y = torch.randn(4, 1, generator=torch.Generator().manual_seed(2))
    for w in model.trainable_weights:
        w.requires_grad_(True)
    loss = ((model(inputs) - y.cuda()) ** 2).mean()
    grads = torch.autograd.grad(loss, model.trainable_weights)
    model.requires_grad_(False)
    refs = []
    for dt in (torch.float32, torch.float64):
        ws = [torch.as_tensor(v, dtype=dt).requires_grad_(True) for v in p]
        er = ref.model_outputs(model, ws, b, dt)["energy"]
        refs.append([g.numpy() for g in torch.autograd.grad(((er - y.to(dt)) ** 2).mean(), ws)])
    _check_weight_grads(model, grads, refs[0], refs[1])
    model.compile(optimizer="adam", loss="mean_squared_error", clipnorm=1.0)
    before = [t.detach().cpu().clone() for t in model.trainable_weights]
    l0 = model.train_on_batch(inputs, y.cuda())
    assert np.isfinite(l0)
    assert all(not torch.equal(u, v.detach().cpu()) for k, (u, v) in enumerate(zip(before, model.trainable_weights))
               if k != CHARGE_LAST_BIAS)


# ------------------------------------------------------------------------------------------- 9. guard
def test_force_training_through_the_solve_raises_and_restores():
    b = _batch(num_graphs=2, seed=91)
    model, _ = _model()
    efm = _efm(model, esp=False)      # no esp inputs named: the wrapper's own esp guard does not fire
    efm.compile(optimizer="adam", loss=["mean_squared_error", "mean_squared_error"])
    e_t = torch.zeros(2, 1).cuda()
    f_t = torch.zeros(len(b["node_number"]), 3).cuda()
    with pytest.raises(NotImplementedError, match="second derivative of the charge equilibration"):
        efm.train_on_batch(_inputs(b), [e_t, f_t])
    assert not any(t.requires_grad for t in model.trainable_weights)
