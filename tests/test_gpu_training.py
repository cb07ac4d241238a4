"""Weight gradients on the engine and ``Model.compile`` / ``train_on_batch`` (kgcnn training/train_qm.py:159-166,
train_citation.py:102-110): the parameter-gradient kernels of csrc/mp_wgrad.hip against float64, SchNet and GCN weight
gradients against torch autograd on the oracles, SGD / Adam trajectories, the fused routes after training, the guard for
layers without weight gradients."""
import numpy as np
import pytest
import torch

from gcnn_keras_amd import synth
from oracle import kgcnn_oracle as ko
from oracle import torch_force_oracle as tfo
from parity import assert_rows_close

pytestmark = pytest.mark.gpu


def _dev(values, splits):
    from gcnn_keras_amd.ragged import RaggedTensor
    return RaggedTensor.from_numpy(values, splits)


def _as_rows(a):
    """Rows as the parity bar sees them: a weight (K, U) has one row per input feature; a bias (U,) is ONE row (its
    entries are sums with cancellation and are measured against the row, as every entry of a dW row is)."""
    a = np.asarray(a)
    return a.reshape(1, -1) if a.ndim == 1 else a


def _close(got, ref32, ref64, what):
    return assert_rows_close(_as_rows(got), _as_rows(ref32), _as_rows(ref64), what=what)


def _wgrad(x, g, bias=True):
    from gcnn_keras_amd.autograd import dense_wgrad
    return dense_wgrad(x, g, with_bias=bias)


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("r,k,u", [(26190, 20, 128), (26190, 128, 128), (2708, 1433, 64), (2301, 64, 128), (65, 3, 7),
                                   (1, 1, 1), (1_200_000, 5, 3)])
def test_dense_wgrad_kernel(r, k, u):
    gen = torch.Generator().manual_seed(r + k + u)
    x = torch.randn(r, k, generator=gen, dtype=torch.float32)
    g = torch.randn(r, u, generator=gen, dtype=torch.float32)
    dw, db = _wgrad(x.cuda(), g.cuda())
    ref64 = x.double().t() @ g.double()
    ref32 = x.t() @ g
    assert_rows_close(dw.cpu().numpy(), ref32.numpy(), ref64.numpy(), what="dW %s" % ((r, k, u),))
    _close(db.cpu().numpy(), g.sum(0).numpy(), g.double().sum(0).numpy(), what="db %s" % ((r, k, u),))


def test_dense_wgrad_zero_rows_and_streams():
    x = torch.zeros(0, 20, device="cuda")
    g = torch.zeros(0, 128, device="cuda")
    dw, db = _wgrad(x, g)
    torch.cuda.synchronize()
    assert torch.count_nonzero(dw).item() == 0 and torch.count_nonzero(db).item() == 0 and tuple(dw.shape) == (20, 128)
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(26190, 128, generator=gen).cuda()
    g = torch.randn(26190, 128, generator=gen).cuda()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        a = _wgrad(x, g)
    with torch.cuda.stream(s2):
        b = _wgrad(x, g)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_embedding_and_softmax_gradients():
    from gcnn_keras_amd.autograd import Embedding, Softmax
    gen = torch.Generator().manual_seed(5)
    numbers = torch.tensor(np.random.default_rng(5).choice([1, 6, 7, 8, 9, 120, -3], size=3000), dtype=torch.float32)
    table = torch.randn(95, 64, generator=gen)
    g = torch.randn(3000, 64, generator=gen)
    tab = table.cuda().requires_grad_(True)
    out = Embedding.apply(numbers.cuda(), tab)
    out.backward(g.cuda())
    ids = numbers.to(torch.int64)
    ok = (ids >= 0) & (ids < 95)
    ref64 = torch.zeros(95, 64, dtype=torch.float64).index_add_(0, ids[ok], g.double()[ok])
    ref32 = torch.zeros(95, 64).index_add_(0, ids[ok], g[ok])
    assert_rows_close(tab.grad.cpu().numpy(), ref32.numpy(), ref64.numpy(), what="embedding table gradient")
    assert torch.count_nonzero(tab.grad[0]).item() == 0

    z = torch.randn(2708, 7, generator=gen)
    gy = torch.randn(2708, 7, generator=gen)
    zd = z.cuda().requires_grad_(True)
    Softmax.apply(zd).backward(gy.cuda())
    refs = []
    for dt in (torch.float32, torch.float64):
        zz = z.detach().clone().to(dt).requires_grad_(True)
        torch.softmax(zz, -1).backward(gy.to(dt))
        refs.append(zz.grad.numpy())
    assert_rows_close(zd.grad.cpu().numpy(), refs[0], refs[1], what="softmax gradient")


# ---------------------------------------------------------------------------------------------------------------- SchNet
def _schnet_setup(num_graphs=128, seed=1234):
    from gcnn_keras_amd.literature import Schnet
    b = synth.qm9_like_batch(num_graphs, seed=seed)
    p = synth.schnet_params(random_bias=True)
    model = Schnet.make_model(depth=3)
    model.set_weights(list(p.values()))
    inputs = [_dev(b["node_number"], b["node_splits"]), _dev(b["node_coordinates"], b["node_splits"]),
              _dev(b["edge_indices"], b["edge_splits"])]
    return b, p, model, inputs


def _oracle_energy(pt, b, dtype):
    return tfo.schnet_energy(pt, b["node_number"], torch.from_numpy(b["node_coordinates"]).to(dtype),
                             b["edge_indices"], b["node_splits"], b["edge_splits"], depth=3)


def _oracle_grads(params, b, target, dtype):
    pt = {k: v.requires_grad_(True) for k, v in tfo.to_torch(params, dtype).items()}
    e = _oracle_energy(pt, b, dtype)
    loss = (e - torch.from_numpy(target).to(dtype)).abs().mean()
    loss.backward()
    return float(loss), {k: v.grad.numpy() for k, v in pt.items()}


def test_schnet_weight_gradients():
    b, p, model, inputs = _schnet_setup()
    with torch.no_grad():
        e0 = model(inputs).cpu().numpy()
    target = (e0 + 0.37 + 0.1 * np.sin(np.arange(e0.shape[0]))[:, None]).astype(np.float32)  # pred - y < 0 everywhere
    model.requires_grad_(True)
    model.fused.last = None
    pred = model(inputs)
    assert model.fused.last is None                 # weights that require grad: the layer path served the call
    loss = (pred - torch.from_numpy(target).cuda()).abs().mean()
    loss.backward()
    got = {n: t.grad.cpu().numpy() for n, t in zip(p, model.trainable_weights)}
    model.requires_grad_(False)
    _, g32 = _oracle_grads(p, b, target, torch.float32)
    _, g64 = _oracle_grads(p, b, target, torch.float64)
    assert set(got) == set(g64) and "embedding" in got
    for name in p:
        _close(got[name], g32[name], g64[name], what="dL/d " + name)


def test_schnet_sgd_trajectory_matches_oracle():
    b, p, model, inputs = _schnet_setup(num_graphs=32, seed=21)
    rng = np.random.default_rng(4)
    target = rng.normal(size=(32, 1)).astype(np.float32)
    model.compile(optimizer="sgd", loss="mean_absolute_error")
    losses = [model.train_on_batch(inputs, target) for _ in range(10)]
    assert not any(t.requires_grad for t in model.trainable_weights)
    ref = tfo.to_torch(p, torch.float64)
    ref = {k: v.requires_grad_(True) for k, v in ref.items()}
    opt = torch.optim.SGD(list(ref.values()), lr=0.01)
    ref_losses = []
    for _ in range(10):
        opt.zero_grad()
        loss = (_oracle_energy(ref, b, torch.float64) - torch.from_numpy(target).double()).abs().mean()
        loss.backward()
        opt.step()
        ref_losses.append(float(loss))
    np.testing.assert_allclose(losses, ref_losses, rtol=1e-5)
    for (name, t), a in zip(ref.items(), model.get_weights()):
        ref_w = t.detach().numpy()
        assert np.max(np.abs(a - ref_w)) <= 1e-5 * max(float(np.max(np.abs(ref_w))), 1e-3), name


def test_schnet_adam_reduces_loss_and_is_deterministic():
    def run():
        b, p, model, inputs = _schnet_setup(num_graphs=32, seed=21)
        target = np.random.default_rng(4).normal(size=(32, 1)).astype(np.float32)
        model.compile(optimizer="adam", loss="mean_absolute_error")
        losses = [model.train_on_batch(inputs, target) for _ in range(30)]
        return losses, model.get_weights()

    l1, w1 = run()
    l2, w2 = run()
    assert l1[-1] < 0.8 * l1[0], l1
    assert l1 == l2
    for a, c in zip(w1, w2):
        assert np.array_equal(a, c)


def test_routes_after_training():
    from gcnn_keras_amd.engine import GraphedModel
    b, p, model, inputs = _schnet_setup(num_graphs=32, seed=21)
    b2 = synth.qm9_like_batch(16, seed=77)
    inputs2 = [_dev(b2["node_number"], b2["node_splits"]), _dev(b2["node_coordinates"], b2["node_splits"]),
               _dev(b2["edge_indices"], b2["edge_splits"])]
    with torch.no_grad():
        model(inputs)
        model(inputs)                               # the slot's graph is captured before training
        model.fused.call_group([inputs, inputs2])
        model.fused.call_group([inputs, inputs2])
    graphed = GraphedModel(model, inputs, grad=False)
    target = np.random.default_rng(4).normal(size=(32, 1)).astype(np.float32)
    model.compile(optimizer="adam", loss="mean_absolute_error")
    model.fused.last = None
    for _ in range(3):
        model.train_on_batch(inputs, target)
    assert model.fused.last is None                # the steps took the layer path
    names = list(p)
    trained = dict(zip(names, model.get_weights()))
    assert not np.array_equal(trained["interaction0/cfconv/dense1/kernel"], p["interaction0/cfconv/dense1/kernel"])

    def ref(batch, dtype):
        return _oracle_energy(tfo.to_torch(trained, dtype), batch, dtype).detach().numpy()

    r32, r64 = ref(b, torch.float32), ref(b, torch.float64)
    with torch.no_grad():
        for expect in ("graph", "graph"):
            out = model(inputs).cpu().numpy()
            assert model.fused.last == expect
            assert_rows_close(out, r32, r64, what="fused route after training (no_grad)")
    out = model(inputs).cpu().numpy()               # plain call, grad mode, weights frozen again
    assert model.fused.last in ("direct", "graph")
    assert_rows_close(out, r32, r64, what="fused route after training (plain call)")
    with torch.no_grad():
        grp = model.fused.call_group([inputs, inputs2])
    assert_rows_close(grp[0].cpu().numpy(), r32, r64, what="call_group member 0 after training")
    assert_rows_close(grp[1].cpu().numpy(), ref(b2, torch.float32), ref(b2, torch.float64),
                      what="call_group member 1 after training")
    out = graphed().cpu().numpy()
    assert_rows_close(out, r32, r64, what="GraphedModel captured before training")


def test_layer_path_graph_sees_new_filter_weights():
    """A HIP graph captured around a fused cfconv on the layer path reads SchNetCFconv's packed filter image: an
    in-place weight update after the capture reaches the replay."""
    from gcnn_keras_amd.engine import GraphedModel
    from gcnn_keras_amd.layers.conv.schnet_conv import SchNetInteraction
    from gcnn_keras_amd.layers.geom import GaussBasisLayer, NodeDistanceEuclidean, NodePosition
    from gcnn_keras_amd.model.utils import Model
    b = synth.qm9_like_batch(8, seed=3)
    inter = SchNetInteraction(units=128)
    inter.ensure_built([(None, None, 128), (None, None, 20), (None, None, 2)])
    xyz, edi = _dev(b["node_coordinates"], b["node_splits"]), _dev(b["edge_indices"], b["edge_splits"])
    with torch.no_grad():
        ed = GaussBasisLayer(bins=20, distance=4, offset=0.0, sigma=0.4)(NodeDistanceEuclidean()(NodePosition()([xyz, edi])))
    node = _dev(np.random.default_rng(1).normal(size=(int(b["node_splits"][-1]), 128)).astype(np.float32),
                b["node_splits"])
    probe = Model("probe", lambda x: inter(x).values, [inter])
    with torch.no_grad():
        graphed = GraphedModel(probe, [node, ed, edi], grad=False)
        inter.lay_cfconv.lay_dense1.kernel.mul_(1.5)
        inter.lay_cfconv.lay_dense2.bias.add_(0.25)
        replay = graphed().clone()
        eager = inter([node, ed, edi]).values
    assert inter.lay_cfconv._packed is not None
    assert torch.equal(replay, eager)


# ---------------------------------------------------------------------------------------------------------------- GCN
def _gcn_torch(p, x, w, idx, n_nodes, depth=3):
    """GCN.make_model with node output [64, 32, 7] softmax (kgcnn/literature/GCN.py:95-109) in torch: one graph, so the
    sample indices are the batch indices."""
    recv, send = idx[:, 0], idx[:, 1]
    n = x @ p["dense0/kernel"] + p["dense0/bias"]
    for i in range(depth):
        no = n @ p["gcn%d/kernel" % i] + p["gcn%d/bias" % i]
        msg = no.index_select(0, send) * w
        n = torch.relu(torch.zeros((n_nodes, no.shape[1]), dtype=no.dtype).index_add_(0, recv, msg))
    n = torch.relu(n @ p["output_mlp/0/kernel"] + p["output_mlp/0/bias"])
    n = torch.relu(n @ p["output_mlp/1/kernel"] + p["output_mlp/1/bias"])
    return torch.softmax(n @ p["output_mlp/2/kernel"] + p["output_mlp/2/bias"], dim=-1)


def test_gcn_weight_gradients():
    from gcnn_keras_amd.literature import GCN
    from gcnn_keras_amd.model.losses import categorical_crossentropy
    g = synth.cora_like_graph()
    p = synth.gcn_params(seed=9, in_features=1433, random_bias=True)
    model = GCN.make_model(
        inputs=[{"shape": (None, 1433), "name": "node_attributes", "dtype": "float32", "ragged": True},
                {"shape": (None, 1), "name": "edge_weights", "dtype": "float32", "ragged": True},
                {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True}],
        gcn_args={"units": 64, "use_bias": True, "activation": "relu", "pooling_method": "sum"},
        depth=3, output_embedding="node", output_to_tensor=False,
        output_mlp={"use_bias": [True, True, True], "units": [64, 32, 7], "activation": ["relu", "relu", "softmax"]})
    model.set_weights(list(p.values()))
    n = int(g["node_splits"][-1])
    rng = np.random.default_rng(17)
    labels = np.eye(7, dtype=np.float32)[rng.integers(0, 7, size=n)]
    mask = np.zeros(n, np.float32)
    mask[rng.choice(n, size=140, replace=False)] = 1.0
    inputs = [_dev(g["node_attributes"], g["node_splits"]), _dev(g["edge_weights"], g["edge_splits"]),
              _dev(g["edge_indices"], g["edge_splits"])]

    def reference(dtype):
        pt = {k: v.requires_grad_(True) for k, v in tfo.to_torch(p, dtype).items()}
        out = _gcn_torch(pt, torch.from_numpy(g["node_attributes"]).to(dtype),
                         torch.from_numpy(g["edge_weights"]).to(dtype), torch.from_numpy(g["edge_indices"]), n)
        loss = categorical_crossentropy(out, torch.from_numpy(labels).to(dtype), torch.from_numpy(mask).to(dtype))
        loss.backward()
        return out.detach().numpy(), float(loss), {k: v.grad.numpy() for k, v in pt.items()}

    out64, loss64, g64 = reference(torch.float64)
    _, loss32, g32 = reference(torch.float32)
    # the restatement is first held to the reference's forward
    oracle = ko.gcn_forward(ko.to_dtype(p, np.float64), ko.R(g["node_attributes"].astype(np.float64), g["node_splits"]),
                            ko.R(g["edge_weights"].astype(np.float64), g["edge_splits"]),
                            ko.R(g["edge_indices"], g["edge_splits"])).values
    assert np.max(np.abs(out64 - oracle)) <= 1e-12

    model.requires_grad_(True)
    pred = model(inputs)
    loss = categorical_crossentropy(pred, labels, mask)
    loss.backward()
    got = {k: t.grad.cpu().numpy() for k, t in zip(p, model.trainable_weights)}
    model.requires_grad_(False)
    assert abs(float(loss) - loss64) <= 1e-5 * abs(loss64)
    for name in p:
        _close(got[name], g32[name], g64[name], what="GCN dL/d " + name)
    # train_on_batch with the mask as sample_weight: one Adam step moves the loss the same way
    model.compile(optimizer="adam", loss="categorical_crossentropy")
    first = model.train_on_batch(inputs, labels, sample_weight=mask)
    assert abs(first - loss64) <= 1e-5 * abs(loss64)
    with torch.no_grad():
        after = float(categorical_crossentropy(model(inputs), labels, mask))
    assert after < first


# ---------------------------------------------------------------------------------------------------------------- guards
def test_painn_with_trainable_weights_raises():
    from gcnn_keras_amd.literature import PAiNN
    b = synth.md17_like_batch(num_graphs=2, seed=5)
    model = PAiNN.make_model(equiv_initialize_kwargs={"dim": 3, "method": "eps"})
    inputs = [_dev(b["node_number"], b["node_splits"]), _dev(b["node_coordinates"], b["node_splits"]),
              _dev(b["edge_indices"], b["edge_splits"])]
    model.requires_grad_(True)
    with pytest.raises(NotImplementedError):
        model(inputs)
    with torch.no_grad():
        model(inputs)                               # no gradient asked: the fused route serves the call
    model.requires_grad_(False)
    model(inputs)


def test_nothing_leaks_into_inference():
    from gcnn_keras_amd.model.force import EnergyForceModel
    b, p, model, inputs = _schnet_setup(num_graphs=8, seed=5)
    assert not any(t.requires_grad for t in model.trainable_weights)
    efm = EnergyForceModel(model_energy=model, coordinate_input=1, energy_output=0, output_as_dict=True,
                           output_to_tensor=True, output_squeeze_states=True)
    efm(inputs)
    before = efm(inputs)["force"].clone()
    model.compile(optimizer="adam", loss="mean_absolute_error")
    after = efm(inputs)["force"]
    assert torch.equal(before, after)
    assert not any(t.requires_grad for t in model.trainable_weights)
