"""HDNNP2nd on the engine (the fork's force_hdnnp2nd.py): the symmetry-function kernels against the reference's own
known answers and a torch restatement (tests/hdnnp_reference.py), their reverse and forward-mode derivatives, the
relational dense kernels, determinism, the fork's model (energy, forces, graph replay) and its training."""
import os

import numpy as np
import pytest
import torch

import hdnnp_reference as ref
from gcnn_keras_amd import _ffi, synth
from gcnn_keras_amd.layers.conv.acsf_conv import ACSFG2, ACSFG4
from gcnn_keras_amd.layers.relational import relational_dense_raw, relational_dense_t_raw, relational_wgrad
from gcnn_keras_amd.literature import HDNNP2nd
from gcnn_keras_amd.model.force import EnergyForceModel
from gcnn_keras_amd.ragged import RaggedTensor
from parity import assert_forces_close, assert_rows_close

pytestmark = pytest.mark.gpu

FORK = synth.HDNNP_FORK


def _rag(values, splits):
    return RaggedTensor.from_numpy(values, splits)


def _global(idx, idx_splits, node_splits):
    shift = np.repeat(node_splits[:-1], np.diff(idx_splits))
    return idx + shift[:, None]


def _fork_layers():
    kw = synth.hdnnp_model_kwargs()
    g2 = ACSFG2(**ACSFG2.make_param_table(**kw["g2_kwargs"]))
    g4 = ACSFG4(**ACSFG4.make_param_table(**kw["g4_kwargs"]))
    return g2, g4


def _batch(num_graphs=6, seed=5):
    b = synth.hdnnp_batch(num_graphs=num_graphs, seed=seed)
    b["ij"] = _global(b["edge_indices"], b["edge_splits"], b["node_splits"])
    b["ijk"] = _global(b["angle_indices"], b["angle_splits"], b["node_splits"])
    return b


def _inputs(b):
    return [_rag(b["node_number"], b["node_splits"]), _rag(b["node_coordinates"], b["node_splits"]),
            _rag(b["edge_indices"], b["edge_splits"]), _rag(b["angle_indices"], b["angle_splits"])]


def _restate(layer, b, dt, xyz=None):
    t, rmap, pmap = ref.tables(layer)
    x = torch.as_tensor(b["node_coordinates"], dtype=dt) if xyz is None else xyz
    if isinstance(layer, ACSFG4):
        return ref.g4(b["node_number"], x, b["ijk"], t, rmap, pmap, layer.num_relations, layer.multiplicity,
                      layer.num_centers)
    return ref.g2(b["node_number"], x, b["ij"], t, rmap, layer.num_relations, layer.num_centers)


def _engine(layer, b, xyz=None):
    z = _rag(b["node_number"], b["node_splits"])
    x = _rag(b["node_coordinates"], b["node_splits"]) if xyz is None else xyz
    idx = _rag(b["angle_indices"], b["angle_splits"]) if isinstance(layer, ACSFG4) else \
        _rag(b["edge_indices"], b["edge_splits"])
    return layer([z, x, idx])


# ------------------------------------------------------------------------------------------- reference known answers
def test_reference_known_answers(golden_dir):
    d = np.load(os.path.join(golden_dir, "acsf_reference_case.npz"))
    ns = d["node_splits"]
    z, x = _rag(d["node_number"], ns), _rag(d["node_coordinates"], ns)
    ei = _rag(d["edge_indices"], d["edge_splits"])
    g2 = ACSFG2(**ACSFG2.make_param_table(eta=[0.0, 0.3], rs=[0.0, 3.0], rc=10.0, elements=[1, 6, 16]))
    out2 = g2([z, x, ei]).values.cpu().numpy()
    assert np.all(np.abs(out2[ns[2]] - d["g2_expected_last_first"]) < 1e-4)
    tri, tri_len = [], []
    for g in range(len(ns) - 1):
        t = synth.angle_indices(d["edge_indices"][d["edge_splits"][g]:d["edge_splits"][g + 1]], edge_pairing="ik")
        tri.append(t)
        tri_len.append(len(t))
    ijk = _rag(np.concatenate(tri), np.concatenate([[0], np.cumsum(tri_len)]).astype(np.int64))
    g4 = ACSFG4(**ACSFG4.make_param_table(eta=[0.0, 0.3], lamda=[-1.0, 1.0], rc=6.0, zeta=[1.0, 8.0],
                                          elements=[1, 6, 16], multiplicity=2.0))
    out4 = g4([z, x, ijk]).values.cpu().numpy()
    assert np.all(np.abs(out4[ns[2]] - d["g4_expected_last_first"]) < 1e-4)


# ------------------------------------------------------------------------------------------- forward vs restatement
def _target_set(layer, rng):
    """A rank-4 (target-set) table: the rank-3 table per receiver element, scaled differently per element."""
    t = layer._param_table
    reps = []
    for e in range(len(layer.element_mapping)):
        tt = np.array(t, dtype=np.float64)
        tt[..., 0] *= 1.0 + 0.25 * e
        reps.append(tt)
    return np.stack(reps, 0)


@pytest.mark.parametrize("kind", ["g2", "g4", "g2_target", "g4_target"])
def test_acsf_forward_matches_restatement(kind):
    b = _batch()
    g2, g4 = _fork_layers()
    layer = g2 if kind.startswith("g2") else g4
    if kind.endswith("target"):
        rng = np.random.default_rng(1)
        if layer is g2:
            layer = ACSFG2(eta_rs_rc=_target_set(g2, rng), element_mapping=g2.element_mapping)
        else:
            layer = ACSFG4(eta_zeta_lambda_rc=_target_set(g4, rng), element_mapping=g4.element_mapping,
                           multiplicity=g4.multiplicity)
    got = _engine(layer, b).values.cpu().numpy()
    r32, r64 = (_restate(layer, b, dt).numpy() for dt in (torch.float32, torch.float64))
    assert_rows_close(got, r32, r64, what="ACSF %s" % kind)


def test_unmapped_neighbour_and_tiny_molecules():
    # an element without a table entry (S) contributes nothing; a 1-atom and a 2-atom molecule have no triplets
    g2, g4 = _fork_layers()
    xyz = np.array([[0, 0, 0], [1.5, 0, 0], [0, 1.7, 0.2], [5, 5, 5], [7, 5, 5], [9, 9, 9]], np.float32) * 1.8
    z = np.array([6, 16, 1, 8, 7, 1], np.int64)
    ns = np.array([0, 3, 5, 6], np.int64)
    ij = [np.array([[a, c] for a in range(n) for c in range(n) if a != c], np.int64).reshape(-1, 2)
          for n in (3, 2, 1)]
    ijk = [synth.angle_indices(e) for e in ij]
    b = {"node_number": z, "node_coordinates": xyz, "node_splits": ns,
         "edge_indices": np.concatenate(ij), "edge_splits": np.concatenate([[0], np.cumsum([len(e) for e in ij])]),
         "angle_indices": np.concatenate(ijk).reshape(-1, 3),
         "angle_splits": np.concatenate([[0], np.cumsum([len(t) for t in ijk])])}
    b["ij"] = _global(b["edge_indices"], b["edge_splits"], ns)
    b["ijk"] = _global(b["angle_indices"], b["angle_splits"], ns)
    for layer in (g2, g4):
        got = _engine(layer, b).values.cpu().numpy()
        r64 = _restate(layer, b, torch.float64).numpy()
        assert np.allclose(got, r64, rtol=1e-5, atol=1e-6)
        assert np.all(got[5] == 0.0)
    assert np.all(_engine(g4, b).values.cpu().numpy()[3:] == 0.0)


# ------------------------------------------------------------------------------------------- reverse and JVP
@pytest.mark.parametrize("which", ["g2", "g4"])
def test_acsf_reverse_and_jvp(which):
    b = _batch(num_graphs=3, seed=9)
    g2, g4 = _fork_layers()
    layer = g2 if which == "g2" else g4
    gen = torch.Generator().manual_seed(3)
    width = layer.num_relations * layer.num_functions
    n = len(b["node_number"])
    g = torch.randn(n, width, generator=gen)
    h = torch.randn(n, 3, generator=gen)
    # engine: reverse (dx), JVP (g_bar) from the adjoint's backward
    xd = torch.as_tensor(b["node_coordinates"]).cuda().requires_grad_(True)
    gd = g.cuda().requires_grad_(True)
    out = _engine(layer, b, xyz=RaggedTensor(xd, torch.as_tensor(b["node_splits"]).cuda())).values
    dx, = torch.autograd.grad(out, xd, grad_outputs=gd, create_graph=True)
    from gcnn_keras_amd.autograd import coordinate_hessian_discarded
    with coordinate_hessian_discarded():
        gbar, = torch.autograd.grad(dx, gd, grad_outputs=h.cuda())
    refs = []
    for dt in (torch.float32, torch.float64):
        x = torch.as_tensor(b["node_coordinates"], dtype=dt).requires_grad_(True)
        gg = g.to(dt).requires_grad_(True)
        rdx, = torch.autograd.grad(_restate(layer, b, dt, xyz=x), x, grad_outputs=gg, create_graph=True)
        rgb, = torch.autograd.grad(rdx, gg, grad_outputs=h.to(dt))
        refs.append((rdx.detach().numpy(), rgb.detach().numpy()))
    assert_rows_close(dx.detach().cpu().numpy(), refs[0][0], refs[1][0], what="%s reverse dx" % which)
    assert_rows_close(gbar.cpu().numpy(), refs[0][1], refs[1][1], what="%s jvp g_bar" % which)


def test_hessian_through_acsf_raises():
    b = _batch(num_graphs=2)
    g2, _ = _fork_layers()
    xd = torch.as_tensor(b["node_coordinates"]).cuda().requires_grad_(True)
    out = _engine(g2, b, xyz=RaggedTensor(xd, torch.as_tensor(b["node_splits"]).cuda())).values
    dx, = torch.autograd.grad(out.sum(), xd, create_graph=True)
    with pytest.raises(NotImplementedError):
        torch.autograd.grad(dx.sum(), xd)


# ------------------------------------------------------------------------------------------- relational dense
def test_relational_dense_kernels():
    gen = torch.Generator().manual_seed(11)
    rows, k, u, nrel = 3000, 640, 35, 30
    x = torch.randn(rows, k, generator=gen)
    w = torch.randn(nrel, k, u, generator=gen) * 0.05
    bias = torch.randn(u, generator=gen) * 0.1
    rel = torch.randint(0, 10, (rows,), generator=gen)
    rel[::97] = 40          # outside the table: zero kernel
    rel[5] = -3
    g = torch.randn(rows, u, generator=gen)
    xd, wd, bd, rd, gd = x.cuda(), w.cuda(), bias.cuda(), rel.cuda(), g.cuda()
    pre, y = relational_dense_raw(xd, wd, bd, rd, 6, 0.0, keep_pre=True)
    dx = relational_dense_t_raw(gd, wd, rd, 6, 0.0, pre)
    dw, db = relational_wgrad(xd, gd, rd, nrel)
    refs = []
    for dt in (torch.float32, torch.float64):
        xx, ww, bb = x.to(dt).requires_grad_(True), w.to(dt).requires_grad_(True), bias.to(dt).requires_grad_(True)
        yy = ref.relational_dense(xx, ww, bb, rel.numpy(), "tanh")
        lin = ref.relational_dense(xx, ww, None, rel.numpy(), "linear")
        gx, = torch.autograd.grad(yy, xx, grad_outputs=g.to(dt))
        gw, gb = torch.autograd.grad(lin, [ww, xx], grad_outputs=g.to(dt))[0], g.to(dt).sum(0)
        refs.append((yy.detach().numpy(), gx.numpy(), gw.numpy(), gb.numpy()))
    assert_rows_close(y.cpu().numpy(), refs[0][0], refs[1][0], what="relational dense y")
    assert_rows_close(dx.cpu().numpy(), refs[0][1], refs[1][1], what="relational dense dx")
    assert_rows_close(dw.cpu().numpy().reshape(-1, u), refs[0][2].reshape(-1, u), refs[1][2].reshape(-1, u),
                      what="relational dense dW")
    assert_rows_close(db.cpu().numpy()[None], refs[0][3][None], refs[1][3][None], what="relational dense db")
    out_rows = (rel < 0) | (rel >= nrel)
    assert torch.equal(y.cpu()[out_rows], torch.tanh(bias).expand(int(out_rows.sum()), u))


# ------------------------------------------------------------------------------------------- determinism
def test_deterministic_runs_and_streams():
    b = _batch(num_graphs=8, seed=21)
    _, g4 = _fork_layers()
    gen = torch.Generator().manual_seed(4)
    g = torch.randn(len(b["node_number"]), g4.num_relations * g4.num_functions, generator=gen).cuda()
    x = torch.randn(3000, 64, generator=gen).cuda()
    gg = torch.randn(3000, 35, generator=gen).cuda()
    rel = torch.randint(0, 9, (3000,), generator=gen).cuda()

    def run():
        xd = torch.as_tensor(b["node_coordinates"]).cuda().requires_grad_(True)
        out = _engine(g4, b, xyz=RaggedTensor(xd, torch.as_tensor(b["node_splits"]).cuda())).values
        dx, = torch.autograd.grad(out, xd, grad_outputs=g)
        dw, db = relational_wgrad(x, gg, rel, 30)
        torch.cuda.synchronize()
        return [t.detach().cpu() for t in (out, dx, dw, db)]

    a = run()
    bb = run()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c = run()
    torch.cuda.synchronize()
    for u, v, w in zip(a, bb, c):
        assert torch.equal(u, v) and torch.equal(u, w)


# ------------------------------------------------------------------------------------------- full model
def _model(seed=10):
    model = HDNNP2nd.make_model_behler(**synth.hdnnp_model_kwargs())
    p = synth.hdnnp_params(seed=seed)
    model.set_weights(list(p.values()))
    return model, p


def _ref_energy(model, p, b, dt, xyz=None):
    x = torch.as_tensor(b["node_coordinates"], dtype=dt) if xyz is None else xyz
    ws = [torch.as_tensor(v, dtype=dt) for v in p.values()]
    return ref.energy(model, ws, b["node_number"], x, b["ij"], b["ijk"], b["node_splits"])


def test_fork_model_energy_forces_and_replay():
    b = _batch(num_graphs=8, seed=31)
    model, p = _model()
    inputs = _inputs(b)
    e_eager = model(inputs)
    r = [_ref_energy(model, p, b, dt).numpy() for dt in (torch.float32, torch.float64)]
    assert_rows_close(e_eager.cpu().numpy(), r[0], r[1], what="HDNNP2nd energy")
    e2 = model(inputs)       # second call: captured
    e3 = model(inputs)       # replayed
    assert model.last_route == "graph"
    assert torch.equal(e3, e_eager) and torch.equal(e2, e_eager)
    efm = EnergyForceModel(model_energy=model, energy_output=0, output_as_dict=False, output_to_tensor=False,
                           output_squeeze_states=True, is_physical_force=False)
    eng, force = efm(inputs)
    refs = []
    for dt in (torch.float32, torch.float64):
        x = torch.as_tensor(b["node_coordinates"], dtype=dt).requires_grad_(True)
        e = _ref_energy(model, p, b, dt, xyz=x)
        f, = torch.autograd.grad(e.sum(), x)
        refs.append(f.numpy())
    assert_forces_close(force.values.cpu().numpy(), refs[0], refs[1], b["node_splits"], what="HDNNP2nd forces")
    # the create_graph pass of training gives the inference tape's forces bit for bit
    _, _, de_dr = efm._tape(inputs, {}, create_graph=True)
    assert torch.equal(de_dr.detach(), force.values)


# A kernel gradient sums the rows of ~1000 atoms of one element; two float32 evaluations of such a sum differ by up to
# ~2x their distance from float64.  The engine must stay within 4x the float32 oracle's distance from float64
# (assert_rows_close) and within this bar of the oracle itself (widest training bars 3.8e-5).
GRAD_RTOL = 4e-5


def test_train_on_batch_weight_gradients():
    b = _batch(num_graphs=6, seed=41)
    model, p = _model()
    inputs = _inputs(b)
    y = torch.randn(6, 1, generator=torch.Generator().manual_seed(2)).cuda()
    for t in model.trainable_weights:
        t.requires_grad_(True)
    e = model(inputs)
    loss = ((e - y) ** 2).mean()
    grads = torch.autograd.grad(loss, model.trainable_weights)
    model.requires_grad_(False)
    refs = []
    for dt in (torch.float32, torch.float64):
        ws = [torch.as_tensor(v, dtype=dt).requires_grad_(True) for v in p.values()]
        er = ref.energy(model, ws, b["node_number"], torch.as_tensor(b["node_coordinates"], dtype=dt), b["ij"],
                        b["ijk"], b["node_splits"])
        lr = ((er - y.cpu().to(dt)) ** 2).mean()
        refs.append([gr.numpy() for gr in torch.autograd.grad(lr, ws)])
    for (name, _), gg, r32, r64 in zip(model.weights, grads, refs[0], refs[1]):
        width = gg.shape[-1]
        assert_rows_close(gg.cpu().numpy().reshape(-1, width), r32.reshape(-1, width), r64.reshape(-1, width),
                          what="dLoss/d" + name, rtol=GRAD_RTOL)


# d(F.R)/dW differentiates the 640 symmetry functions twice; the float32 restatement itself lands up to ~6e-5 of a row
# from float64 there, so the engine's bar (4x that distance) may exceed the default cap of tests/parity.py.
FORCE_GRAD_CAP = 2e-4


def test_force_loss_weight_gradients():
    # d(F . R)/dw for every weight against the restatement differentiated twice
    b = _batch(num_graphs=4, seed=51)
    model, p = _model()
    inputs = _inputs(b)
    gen = torch.Generator().manual_seed(6)
    rr = torch.randn(len(b["node_number"]), 3, generator=gen)
    efm = EnergyForceModel(model_energy=model, energy_output=0, output_as_dict=False, output_squeeze_states=True,
                           is_physical_force=False)
    model.requires_grad_(True)
    try:
        with torch.enable_grad():
            _, _, de_dr = efm._tape(inputs, {}, create_graph=True)
            from gcnn_keras_amd.autograd import coordinate_hessian_discarded
            with coordinate_hessian_discarded():
                # the last bias shifts every energy by a constant: no force depends on it (its gradient is None)
                grads = torch.autograd.grad((de_dr * rr.cuda()).sum(), model.trainable_weights, allow_unused=True)
    finally:
        model.requires_grad_(False)
    refs = []
    for dt in (torch.float32, torch.float64):
        ws = [torch.as_tensor(v, dtype=dt).requires_grad_(True) for v in p.values()]
        x = torch.as_tensor(b["node_coordinates"], dtype=dt).requires_grad_(True)
        er = ref.energy(model, ws, b["node_number"], x, b["ij"], b["ijk"], b["node_splits"])
        f, = torch.autograd.grad(er.sum(), x, create_graph=True)
        gws = torch.autograd.grad((f * rr.to(dt)).sum(), ws, allow_unused=True)
        refs.append([np.zeros(tuple(w_.shape)) if gr is None else gr.numpy() for w_, gr in zip(ws, gws)])
    assert grads[-1] is None
    for (name, _), gg, r32, r64 in zip(model.weights[:-1], grads[:-1], refs[0][:-1], refs[1][:-1]):
        width = gg.shape[-1]
        assert_rows_close(gg.cpu().numpy().reshape(-1, width), r32.reshape(-1, width), r64.reshape(-1, width),
                          what="d(F.R)/d" + name, rtol=GRAD_RTOL, cap=FORCE_GRAD_CAP)


def _force_targets(b, seed):
    rng = np.random.default_rng(seed)
    e = torch.as_tensor(rng.normal(size=(len(b["node_splits"]) - 1, 1)).astype(np.float32))
    f = torch.as_tensor(rng.normal(size=(len(b["node_number"]), 3)).astype(np.float32) * 0.01)
    return e, f


def test_energy_force_sgd_tracks_float64():
    b = _batch(num_graphs=4, seed=61)
    model, p = _model()
    inputs = _inputs(b)
    e_t, f_t = _force_targets(b, 1)
    lr, w_e, w_f = 0.01, 1 / 200, 199 / 200
    efm = EnergyForceModel(model_energy=model, energy_output=0, output_as_dict=False, output_squeeze_states=True,
                           is_physical_force=False)
    efm.compile(optimizer=torch.optim.SGD(model.trainable_weights, lr=lr),
                loss=["mean_squared_error", "mean_squared_error"], loss_weights=[w_e, w_f])
    got = [efm.train_on_batch(inputs, [e_t.cuda(), f_t.cuda()])[0] for _ in range(3)]
    ws = [torch.as_tensor(v, dtype=torch.float64).requires_grad_(True) for v in p.values()]
    want = []
    for _ in range(3):
        x = torch.as_tensor(b["node_coordinates"], dtype=torch.float64).requires_grad_(True)
        er = ref.energy(model, ws, b["node_number"], x, b["ij"], b["ijk"], b["node_splits"])
        f, = torch.autograd.grad(er.sum(), x, create_graph=True)
        total = w_e * ((er - e_t.double()) ** 2).mean() + w_f * ((f - f_t.double()) ** 2).mean()
        want.append(float(total.detach()))
        gs = torch.autograd.grad(total, ws)
        with torch.no_grad():
            for w_, g_ in zip(ws, gs):
                w_ -= lr * g_
    assert np.allclose(got, want, rtol=1e-4), (got, want)
    for (name, t), w64, w0 in zip(model.weights, ws, p.values()):
        moved = w64.detach().numpy() - w0
        diff = t.detach().cpu().numpy() - w64.detach().numpy()
        assert np.abs(diff).max() <= 1e-3 * max(np.abs(moved).max(), 1e-12), name


def test_energy_force_adam_clipnorm_lowers_loss_and_is_deterministic():
    b = _batch(num_graphs=4, seed=71)
    e_t, f_t = _force_targets(b, 2)
    runs = []
    for _ in range(2):
        model, _ = _model()
        efm = EnergyForceModel(model_energy=model, energy_output=0, output_as_dict=False, output_squeeze_states=True,
                               is_physical_force=False)
        efm.compile(optimizer="adam", loss=["mean_squared_error", "mean_squared_error"],
                    loss_weights=[1 / 200, 199 / 200], clipnorm=1.0)
        inputs = _inputs(b)
        losses = [efm.train_on_batch(inputs, [e_t.cuda(), f_t.cuda()])[0] for _ in range(5)]
        runs.append((losses, [t.detach().cpu().clone() for t in model.trainable_weights]))
    assert runs[0][0][-1] < runs[0][0][0]
    assert runs[0][0] == runs[1][0]
    for u, v in zip(runs[0][1], runs[1][1]):
        assert torch.equal(u, v)
