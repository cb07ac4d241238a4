"""Training SchNet on energies and forces (the fork's force_schnet.py:163-205, 262: ``EnergyForceModel`` compiled with an
energy MSE and a force MSE weighted [1/200, 199/200]): the second-derivative kernels of csrc/mp_backward2.hip against
torch float64 double backward, the twice-differentiable reverse rules against the oracle differentiated twice, forces of a
``create_graph`` pass against the inference tape, ``EnergyForceModel.train_on_batch`` against the oracle's SGD
trajectory, the routes after training, and the guards."""
import numpy as np
import pytest
import torch

from gcnn_keras_amd import _ffi, synth
from oracle import torch_force_oracle as tfo
from parity import assert_rows_close
from test_gpu_forces import FORK_SCHNET

pytestmark = pytest.mark.gpu

ACT_NAMES = {0: "linear", 1: "relu", 2: "shifted_softplus", 3: "softplus", 4: "swish", 5: "sigmoid", 6: "tanh",
             7: "leaky_relu", 8: "softplus2", 9: "selu"}
ALPHA = 0.3   # leaky relu slope


def _act(code, v):
    fn = torch.nn.functional
    if code == 0:
        return v
    if code == 1:
        return torch.relu(v)
    if code == 2:
        return fn.softplus(v, threshold=50.0) - np.log(2.0)
    if code == 3:
        return fn.softplus(v, threshold=50.0)
    if code == 4:
        return v * torch.sigmoid(v)
    if code == 5:
        return torch.sigmoid(v)
    if code == 6:
        return torch.tanh(v)
    if code == 7:
        return torch.where(v >= 0, v, ALPHA * v)
    if code == 8:
        return torch.relu(v) + torch.log(0.5 * torch.exp(-v.abs()) + 0.5)
    return 1.05070098 * torch.where(v > 0, v, 1.67326324 * (torch.exp(v) - 1.0))


def _rows(a, width=16):
    a = np.asarray(a)
    return a.reshape(-1, width) if a.ndim == 1 else a


def _double_backward(fn, x, g, h):
    """Reverse of y = g * d fn / dx at (x, g) for the upstream h: (x_bar, g_bar) in x's dtype."""
    x = x.clone().requires_grad_(True)
    g = g.clone().requires_grad_(True)
    gx, = torch.autograd.grad(fn(x), x, grad_outputs=g, create_graph=True)
    x_bar, g_bar = torch.autograd.grad(gx, [x, g], grad_outputs=h, allow_unused=True)
    x_bar = torch.zeros_like(x) if x_bar is None else x_bar
    return x_bar.detach().numpy(), g_bar.detach().numpy()


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("code", sorted(ACT_NAMES))
def test_activation_grad2_kernel(code):
    gen = torch.Generator().manual_seed(100 + code)
    n = 40000
    pre = torch.randn(n, generator=gen) * 3.0
    g = torch.randn(n, generator=gen)
    h = torch.randn(n, generator=gen)
    dev = [t.cuda() for t in (pre, g, h)]
    pre_bar, g_bar = torch.empty_like(dev[0]), torch.empty_like(dev[0])
    _ffi.call("mp_activation_grad2_f32", code, ALPHA, _ffi.ptr(dev[0]), _ffi.ptr(dev[1]), _ffi.ptr(dev[2]),
              _ffi.ptr(pre_bar), _ffi.ptr(g_bar), n, _ffi.stream())
    only_g = torch.empty_like(dev[0])
    _ffi.call("mp_activation_grad2_f32", code, ALPHA, _ffi.ptr(dev[0]), None, _ffi.ptr(dev[2]), None, _ffi.ptr(only_g),
              n, _ffi.stream())
    refs = [_double_backward(lambda v: _act(code, v), pre.to(dt), g.to(dt), h.to(dt))
            for dt in (torch.float32, torch.float64)]
    what = "act %s" % ACT_NAMES[code]
    assert_rows_close(_rows(pre_bar.cpu().numpy()), _rows(refs[0][0]), _rows(refs[1][0]), what=what + " pre_bar")
    assert_rows_close(_rows(g_bar.cpu().numpy()), _rows(refs[0][1]), _rows(refs[1][1]), what=what + " g_bar")
    assert torch.equal(only_g, g_bar)


@pytest.mark.parametrize("bins,distance,sigma", [(25, 5.0, 0.4), (20, 4.0, 0.4)])
def test_gauss_basis_grad2_kernel(bins, distance, sigma):
    gen = torch.Generator().manual_seed(bins)
    m = 30000
    d = torch.rand(m, 1, generator=gen) * (distance + 1.0)
    g = torch.randn(m, bins, generator=gen)
    h = torch.randn(m, 1, generator=gen)
    dd, gd, hd = d.cuda(), g.cuda(), h.cuda()
    d_bar, g_bar = torch.empty_like(dd), torch.empty_like(gd)
    _ffi.call("mp_gauss_basis_grad2_f32", _ffi.ptr(dd), m, bins, distance, sigma, 0.0, _ffi.ptr(gd), _ffi.ptr(hd),
              _ffi.ptr(d_bar), _ffi.ptr(g_bar), _ffi.stream())

    def basis(dt):
        mu = torch.arange(bins, dtype=dt) / float(bins) * float(distance)
        gamma = 1.0 / sigma / sigma / 2.0
        return lambda v: torch.exp(((v - 0.0) - mu).square() * (-gamma))

    refs = [_double_backward(basis(dt), d.to(dt), g.to(dt), h.to(dt)) for dt in (torch.float32, torch.float64)]
    what = "gauss (%d, %g, %g)" % (bins, distance, sigma)
    # d_bar sums 25 terms (4 gamma^2 u^2 - 2 gamma) phi_k with gamma = 3.125: the float32 rounding of u_k = d - mu_k,
    # amplified by gamma u, puts ANY float32 evaluation ~3e-4 of the row from float64 (the float32 oracle is), above the
    # default cap; the bar stays 2x the oracle's own distance
    assert_rows_close(_rows(d_bar.cpu().numpy()), _rows(refs[0][0]), _rows(refs[1][0]), what=what + " d_bar", cap=1e-3)
    assert_rows_close(g_bar.cpu().numpy(), refs[0][1], refs[1][1], what=what + " g_bar")


@pytest.mark.parametrize("add_eps", [False, True])
@pytest.mark.parametrize("rdc", [(20000, 3, 1), (500, 4, 5)])
def test_euclidean_norm_grad2_kernel(add_eps, rdc):
    r, d, c = rdc
    gen = torch.Generator().manual_seed(r + d + c + int(add_eps))
    x = torch.randn(r, d, c, generator=gen)
    x[0] = 0.0                                   # zero-length rows: the cusp
    x[7, :, 0] = 0.0
    g = torch.randn(r, c, generator=gen)
    h = torch.randn(r, d, c, generator=gen)
    flags = (2 if add_eps else 0) | 4
    xd, gd, hd = x.cuda(), g.cuda(), h.cuda()
    x_bar, g_bar = torch.empty_like(xd), torch.empty_like(gd)
    _ffi.call("mp_euclidean_norm_grad2_f32", _ffi.ptr(xd), _ffi.ptr(gd), _ffi.ptr(hd), r, d, c, flags, _ffi.ptr(x_bar),
              _ffi.ptr(g_bar), _ffi.stream())
    eps = 1e-7 if add_eps else 0.0

    def ref(dt):
        xx = x.to(dt).clone().requires_grad_(True)
        gg = g.to(dt).clone().requires_grad_(True)
        norm = torch.sqrt(xx.square().sum(1) + eps)
        gx, = torch.autograd.grad(norm, xx, grad_outputs=gg, create_graph=True)
        xb, gb = torch.autograd.grad(gx, [xx, gg], grad_outputs=h.to(dt))
        xb, gb = xb.detach().numpy(), gb.detach().numpy()
        if not add_eps:                              # TF: inf / NaN at the cusp; the engine: zero sub-gradient
            cusp = (x.square().sum(1) == 0).numpy()
            xb = np.where(cusp[:, None, :], 0.0, xb)
            gb = np.where(cusp, 0.0, gb)
        return xb.reshape(r, -1), gb

    (x32, g32), (x64, g64) = ref(torch.float32), ref(torch.float64)
    got_x, got_g = x_bar.cpu().numpy(), g_bar.cpu().numpy()
    what = "norm %s add_eps=%s" % (rdc, add_eps)
    assert_rows_close(got_x.reshape(r, -1), x32, x64, what=what + " x_bar")
    assert_rows_close(got_g, g32, g64, what=what + " g_bar")
    if not add_eps:
        assert np.count_nonzero(got_x[0]) == 0 and np.count_nonzero(got_g[0]) == 0
        assert np.count_nonzero(got_x[7, :, 0]) == 0 and got_g[7, 0] == 0.0


# ---------------------------------------------------------------------------------------------------------------- rules
def _fork_case(num_graphs, seed):
    from gcnn_keras_amd.literature import Schnet
    from helpers import dev
    b = synth.md17_like_batch(num_graphs=num_graphs, seed=seed)
    p = synth.schnet_params(seed=7, depth=6, emb_out=128, bins=25, last_units=(128, 64, 1), out_units=(),
                            random_bias=True)
    model = Schnet.make_model(**FORK_SCHNET)
    model.set_weights(list(p.values()))
    inputs = [dev(b["node_number"].astype(np.int64), b["node_splits"]), dev(b["node_coordinates"], b["node_splits"]),
              dev(b["edge_indices"], b["edge_splits"])]
    return b, p, model, inputs


ORACLE_KW = dict(depth=6, gauss_args=FORK_SCHNET["gauss_args"],
                 last_mlp_act=("kgcnn>shifted_softplus",) * 2 + ("linear",), output_mlp_act=())


def _oracle_energy(pt, b, xyz):
    return tfo.schnet_energy(pt, b["node_number"], xyz, b["edge_indices"], b["node_splits"], b["edge_splits"],
                             **ORACLE_KW)


def _as_rows(a):
    a = np.asarray(a)
    return a.reshape(1, -1) if a.ndim == 1 else a


def test_second_order_rules_match_the_oracle():
    """dL/dw and dL/dx for L = sum F * R, F = dE/dx recorded with create_graph: every weight (embedding included) and
    the coordinates, per row, against the oracle differentiated twice in float32 and float64."""
    b, p, model, inputs = _fork_case(16, 5)
    n = int(b["node_splits"][-1])
    rr = np.random.default_rng(3).normal(size=(n, 3)).astype(np.float32)
    model.requires_grad_(True)
    weights = model.trainable_weights
    x = inputs[1].values.detach().clone().requires_grad_(True)
    e = model([inputs[0], inputs[1].with_values(x), inputs[2]])
    f, = torch.autograd.grad(e, x, grad_outputs=torch.ones_like(e), create_graph=True)
    assert f.requires_grad
    loss = (f * torch.from_numpy(rr).cuda()).sum()
    got = torch.autograd.grad(loss, weights + [x], allow_unused=True)   # F does not depend on the last bias
    model.requires_grad_(False)
    got = {name: (torch.zeros_like(w) if t is None else t).cpu().numpy()
           for name, t, w in zip(list(p) + ["x"], got, weights + [x])}

    def reference(dt):
        pt = {k: v.requires_grad_(True) for k, v in tfo.to_torch(p, dt).items()}
        xyz = torch.from_numpy(b["node_coordinates"]).to(dt).requires_grad_(True)
        eng = _oracle_energy(pt, b, xyz)
        ff, = torch.autograd.grad(eng.sum(), xyz, create_graph=True)
        leaves = list(pt.values()) + [xyz]
        grads = torch.autograd.grad((ff * torch.from_numpy(rr).to(dt)).sum(), leaves, allow_unused=True)
        return {name: (torch.zeros_like(w) if t is None else t).detach().numpy()
                for name, t, w in zip(list(pt) + ["x"], grads, leaves)}

    r32, r64 = reference(torch.float32), reference(torch.float64)
    assert "embedding" in got and np.count_nonzero(got["embedding"]) > 0
    for name in got:
        assert_rows_close(_as_rows(got[name]), _as_rows(r32[name]), _as_rows(r64[name]), what="d(F.R)/d " + name)


def test_create_graph_forces_equal_the_inference_tape():
    from gcnn_keras_amd.model.force import EnergyForceModel
    b, p, model, inputs = _fork_case(16, 9)
    efm = EnergyForceModel(model_energy=model, coordinate_input=1, energy_output=0, output_as_dict=False,
                           output_to_tensor=False, output_squeeze_states=True, is_physical_force=False)
    efm.fused = False
    eng_ref, force_ref = efm(inputs)
    model.requires_grad_(True)
    with torch.enable_grad():
        _, eng, de_dr = efm._tape(inputs, {}, create_graph=True)
    model.requires_grad_(False)
    assert de_dr.requires_grad
    assert torch.equal(eng.detach(), eng_ref) and torch.equal(de_dr.detach(), force_ref.values)


# ---------------------------------------------------------------------------------------------------------------- training
LOSS_WEIGHTS = [1 / 200, 199 / 200]


def _targets(b, p, seed):
    """Energies and forces off the model's own by a systematic shift plus noise (the oracle at the start weights)."""
    rng = np.random.default_rng(seed)
    e, f = tfo.schnet_energy_force(p, b, torch.float64, is_physical_force=False, **ORACLE_KW)
    e_t = (e + 0.5 + rng.normal(scale=0.1, size=e.shape)).astype(np.float32)
    f_t = (0.8 * f + rng.normal(scale=0.1 * np.std(f), size=f.shape)).astype(np.float32)
    return e_t, f_t


def _fork_efm(model):
    from gcnn_keras_amd.model.force import EnergyForceModel
    return EnergyForceModel(model_energy=model, coordinate_input=1, energy_output=0, output_as_dict=False,
                            output_to_tensor=True, output_squeeze_states=True, is_physical_force=False)


def _oracle_losses(pt, b, e_t, f_t, dt):
    xyz = torch.from_numpy(b["node_coordinates"]).to(dt).requires_grad_(True)
    eng = _oracle_energy(pt, b, xyz)
    ff, = torch.autograd.grad(eng.sum(), xyz, create_graph=True)
    le = (eng - torch.from_numpy(e_t).to(dt)).square().mean()
    lf = (ff - torch.from_numpy(f_t).to(dt)).square().mean()
    return le * LOSS_WEIGHTS[0] + lf * LOSS_WEIGHTS[1], le, lf


def test_train_on_batch_tracks_the_oracle_sgd_trajectory():
    from helpers import dev
    b, p, model, inputs = _fork_case(16, 21)
    e_t, f_t = _targets(b, p, 4)
    efm = _fork_efm(model)
    # lr 1e-3: with random depth-6 weights Keras' SGD default (0.01) overshoots, in the oracle as well
    efm.compile(optimizer=torch.optim.SGD(efm.trainable_weights, lr=1e-3),
                loss=["mean_squared_error", "mean_squared_error"], loss_weights=LOSS_WEIGHTS)
    y = [e_t, dev(f_t, b["node_splits"])]
    got = [efm.train_on_batch(inputs, y) for _ in range(3)]
    assert not any(t.requires_grad for t in model.trainable_weights)
    ref = {k: v.requires_grad_(True) for k, v in tfo.to_torch(p, torch.float64).items()}
    opt = torch.optim.SGD(list(ref.values()), lr=1e-3)
    ref_losses = []
    for _ in range(3):
        opt.zero_grad()
        total, le, lf = _oracle_losses(ref, b, e_t, f_t, torch.float64)
        total.backward()
        opt.step()
        ref_losses.append([float(total.detach()), float(le.detach()), float(lf.detach())])
    print("[train] engine losses", got, "oracle", ref_losses)
    np.testing.assert_allclose(np.array(got), np.array(ref_losses), rtol=1e-4)
    assert got[-1][0] < got[0][0]
    for (name, t), a in zip(ref.items(), model.get_weights()):
        moved = t.detach().numpy() - p[name]
        err = np.max(np.abs((a - p[name]) - moved))
        # 0.1 % of the displacement, plus the float32 rounding of the stored weights over three updates
        bar = 1e-3 * float(np.max(np.abs(moved))) + 3 * np.finfo(np.float32).eps * float(np.max(np.abs(p[name])))
        assert err <= bar, (name, err, float(np.max(np.abs(moved))))


def test_adam_clipnorm_lowers_the_loss_and_is_deterministic():
    from helpers import dev

    def run():
        b, p, model, inputs = _fork_case(16, 21)
        e_t, f_t = _targets(b, p, 4)
        efm = _fork_efm(model)
        # Adam moves every weight by ~lr per step: at Keras' 1e-3 the random depth-6 model overshoots (the float64
        # oracle's loss rises 0.003 -> 39 at step 2 as well); 1e-5 stays in the descent regime
        efm.compile(optimizer=torch.optim.Adam(efm.trainable_weights, lr=1e-5, eps=1e-7),
                    loss=["mean_squared_error", "mean_squared_error"], loss_weights=LOSS_WEIGHTS, clipnorm=1.0)
        losses = [efm.train_on_batch(inputs, [e_t, dev(f_t, b["node_splits"])]) for _ in range(6)]
        return losses, model.get_weights()

    l1, w1 = run()
    l2, w2 = run()
    print("[train] adam losses", [x[0] for x in l1])
    assert l1[-1][0] < 0.7 * l1[0][0]
    assert l1 == l2
    for a, c in zip(w1, w2):
        assert np.array_equal(a, c)


def test_padded_and_ragged_force_targets_give_the_same_step():
    from helpers import dev
    results = []
    for form in ("ragged", "flat", "padded"):
        b, p, model, inputs = _fork_case(16, 33)
        e_t, f_t = _targets(b, p, 8)
        ns = b["node_splits"]
        if form == "ragged":
            ft = dev(f_t, ns)
        elif form == "flat":
            ft = f_t
        else:
            counts = np.diff(ns)
            ft = np.full((len(counts), int(counts.max()) + 2, 3), 1e3, np.float32)   # padding far off: must not count
            for g in range(len(counts)):
                ft[g, :counts[g]] = f_t[ns[g]:ns[g + 1]]
        efm = _fork_efm(model)
        efm.compile(optimizer="sgd", loss=["mean_squared_error", "mean_squared_error"], loss_weights=LOSS_WEIGHTS)
        results.append((efm.train_on_batch(inputs, [e_t, ft]), model.get_weights()))
    for losses, ws in results[1:]:
        assert losses == results[0][0]
        for a, c in zip(ws, results[0][1]):
            assert np.array_equal(a, c)


def test_routes_serve_the_trained_weights():
    from gcnn_keras_amd.engine import GraphedModel
    from helpers import dev
    b, p, model, inputs = _fork_case(16, 21)
    e_t, f_t = _targets(b, p, 4)
    efm = _fork_efm(model)
    efm.output_to_tensor = False
    efm(inputs)
    efm(inputs)                                      # the fused energy_force route has captured its graph
    assert model.fused.last == "graph"
    graphed = GraphedModel(model, inputs, grad=False)
    efm.compile(optimizer="adam", loss=["mean_squared_error", "mean_squared_error"], loss_weights=LOSS_WEIGHTS,
                clipnorm=1.0)
    for _ in range(3):
        efm.train_on_batch(inputs, [e_t, dev(f_t, b["node_splits"])])
    assert not any(t.requires_grad for t in model.trainable_weights)
    trained = dict(zip(p, model.get_weights()))
    assert not np.array_equal(trained["interaction3/cfconv/dense1/kernel"], p["interaction3/cfconv/dense1/kernel"])
    (e32, f32), (e64, f64) = (tfo.schnet_energy_force(trained, b, dt, is_physical_force=False, **ORACLE_KW)
                              for dt in (torch.float32, torch.float64))
    from parity import assert_forces_close
    model.fused.last = None
    eng, force = efm(inputs)
    assert model.fused.last is not None              # the fused reverse pass served the call
    assert_rows_close(eng.cpu().numpy(), e32, e64, what="fused energy after training")
    assert_forces_close(force.values.cpu().numpy(), f32, f64, b["node_splits"], what="fused forces after training")
    assert_rows_close(graphed().cpu().numpy(), e32, e64, what="GraphedModel captured before training")
    efm.fused = False
    eng, force = efm(inputs)
    assert_forces_close(force.values.cpu().numpy(), f32, f64, b["node_splits"], what="tape forces after training")


# ---------------------------------------------------------------------------------------------------------------- guards
def test_once_differentiable_rules_raise_when_differentiated_twice():
    from gcnn_keras_amd.autograd import Binary, CosCutoff
    d = (torch.rand(1000, 1) * 4.0 + 0.5).cuda().requires_grad_(True)
    y = CosCutoff.apply(d, 5.0)
    z = Binary.apply(y, y, _ffi.MP_MUL)
    gd, = torch.autograd.grad(z.sum(), d, create_graph=True)
    with pytest.raises(RuntimeError, match="differentiate twice"):
        gd.sum().backward()
    a = torch.randn(100, 3).cuda().requires_grad_(True)
    w = torch.randn(100, 1).cuda().requires_grad_(True)
    out = Binary.apply(a, w, _ffi.MP_MUL)
    with pytest.raises(NotImplementedError):
        torch.autograd.grad(out.sum(), a, create_graph=True)
    ga, = torch.autograd.grad(Binary.apply(a, w, _ffi.MP_MUL).sum(), a)      # first order: unchanged
    assert torch.equal(ga, w.expand(100, 3))


def test_painn_force_training_raises():
    from gcnn_keras_amd.literature import PAiNN
    from gcnn_keras_amd.model.force import EnergyForceModel
    from helpers import mol_inputs
    b = synth.md17_like_batch(num_graphs=2, seed=5)
    model = PAiNN.make_model(equiv_initialize_kwargs={"dim": 3, "method": "eps"})
    efm = EnergyForceModel(model_energy=model, coordinate_input=1, energy_output=0, output_as_dict=True,
                           output_squeeze_states=True)
    efm.compile(loss="mean_squared_error")
    n = int(b["node_splits"][-1])
    with pytest.raises(NotImplementedError):
        efm.train_on_batch(mol_inputs(b), [np.zeros((2, 1), np.float32), np.zeros((n, 3), np.float32)])
    assert not any(t.requires_grad for t in model.trainable_weights)
