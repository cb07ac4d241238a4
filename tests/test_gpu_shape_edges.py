"""The EGNN, DimeNet++, ACSF and PaiNN kernels off the molecular shapes (tests/topologies.py): hub receivers whose edges
span many 32-edge tiles, exact tile sizes, the widest and the narrowest encodings and basis widths, every activation
code, absent biases, hundreds of triplets per edge, symmetry-function tables wider than a wave with a cutoff per
function, the width bound, and one graph too large for the LDS-tile message kernels.  Every comparison goes through
``parity.assert_rows_close`` / ``assert_forces_close`` with the caps the family's own test file uses; no cap of its own.

Distance of the float32 torch restatement from its float64 twin on these cases (rowwise_rel, torch CPU; asserted below
half the cap by tests/test_topologies.py, which prints each figure):

  EGNN edge step, hub batch (260 nodes, in-degrees 31 1 32 33 7 64 65 100 1000 | 2 96 5, x = d^2, d in 0.9..10)
    forward 5e-07..1.6e-06, h_bar 9e-07..2.5e-06
    x_bar   9.4e-04..3.0e-03 with the encoding, 1.8e-04..2.8e-04 without; self loops + duplicates 2.8e-03   (ENC_REV_CAP)
  EGNN exact tile sizes (E = 1 31 32 33 64)      forward <= 8e-07, h_bar <= 9e-07, x_bar 1e-05..5e-04
  EGNN encoding widths (43 nodes, 210 edges)     forward <= 2.1e-06, h_bar <= 1.8e-06, x_bar 2e-05 (norm) .. 1.8e-03
  EGNN activations / absent biases               forward <= 3.3e-06, h_bar <= 3.9e-06, x_bar 2e-04..2.2e-03
  EGNN model, 70-atom molecule, cutoff 8 A       forces 4.8e-06 / 1.0e-05 of the molecule's scale, energy 6e-07
  triplet step, 324 edges, up to 1000 per edge   forward, xdown_bar, sbf_bar <= 1.2e-06 (nsbf 7 42 64 65), <= 4.1e-06 (1)
  edge angle reverse, 70 triplets per edge       theta 5.4e-06, v_bar 1.3e-05 sorted / 7.7e-06 shuffled
  ACSF wide tables (70 / 100 functions)          forward <= 4.1e-07, dx <= 2.1e-06, g_bar <= 1.0e-06
  ACSF G2 150 atoms all pairs 4.1e-07 / dx 2.5e-06; 64 and 65 pairs 1.3e-07 / 1.9e-06; G4 40 atoms 8.1e-07 / 3.3e-06
  ACSF G2 4 x 512 functions 1.6e-07 / 6.0e-07; 4 x 171 functions 1.7e-07 / 5.8e-07
  PaiNN, one graph of 5000 points                forces 1.3e-06 of the scale, energy 2.9e-06
"""
import numpy as np
import pytest
import torch

import dimenet_reference as dref
import egnn_reference as eref
import topologies as T
from gcnn_keras_amd import _ffi, synth
from gcnn_keras_amd.layers.conv.acsf_conv import ACSFG2, ACSFG4
from gcnn_keras_amd.layers.conv.dimenet_conv import DimNetInteractionPPBlock, SphericalBasisLayer
from gcnn_keras_amd.layers.conv.egnn_conv import FusedEdgeStep, fused_edge_supported
from gcnn_keras_amd.layers.gather import GatherEmbeddingSelection
from gcnn_keras_amd.layers.geom import EdgeAngle, NodeDistanceEuclidean, NodePosition, PositionEncodingBasisLayer
from gcnn_keras_amd.layers.mlp import GraphMLP
from gcnn_keras_amd.layers.modules import LazyConcatenate, LazyMultiply, LazySubtract
from gcnn_keras_amd.layers.pooling import PoolingLocalEdges
from gcnn_keras_amd.model.force import EnergyForceModel
from gcnn_keras_amd.ragged import RaggedTensor
from helpers import mol_inputs, painn_weight_list
from parity import assert_forces_close, assert_rows_close, rowwise_rel

pytestmark = pytest.mark.gpu

ENC_REV_CAP = 1e-2    # tests/test_gpu_egnn.py: x_bar rows of the edge step (see the table above its ENC_CAP)
SBF_CAP = 1.0         # tests/test_gpu_dimenet.py: spherical-basis rows are held to the float32 restatement's own distance


def _rag(values, splits):
    return RaggedTensor.from_numpy(np.ascontiguousarray(values), splits)


# ====================================================================================================== EGNN
class _OneFrequency:
    """A one-column-pair encoding (K = 1): ``PositionEncodingBasisLayer`` starts at dim_half 2 (its frequency table divides
    by dim_half - 1), the kernel takes any K >= 1; this carries what ``EdgeStepSpec`` reads."""
    dim_half = 1

    def __init__(self, interleave):
        self.interleave_sin_cos = interleave

    def scales(self, device):
        return torch.from_numpy(T.one_frequency_scales()).to(device)


def _step(case):
    """FusedEdgeStep over layers that hold the case's weights."""
    w = case["weights"]
    cols = 2 * case["dim_half"] if case["dim_half"] else 1
    edge_mlp = GraphMLP(units=[128, 128], activation=list(case["acts"]),
                        use_bias=[w["b1"] is not None, w["b2"] is not None])
    edge_mlp.ensure_built((None, None, 256 + cols))
    edge_mlp.set_weights([a for a in (w["w1"], w["b1"], w["w2"], w["b2"]) if a is not None])
    att = None
    if case["attention"]:
        att = GraphMLP(units=1, activation=case["gate"], use_bias=w["ba"] is not None)
        att.ensure_built((None, None, 128))
        att.set_weights([a for a in (w["wa"], w["ba"]) if a is not None])
    if case["dim_half"] == 0:
        enc = None
    elif case["dim_half"] == 1:
        enc = _OneFrequency(case["interleave"])
    else:
        enc = PositionEncodingBasisLayer(dim_half=case["dim_half"], interleave_sin_cos=case["interleave"])
    return FusedEdgeStep(edge_mlp, att, enc)


def _sequence(step, h, x, ei):
    """The reference's layer sequence of the edge step (as tests/test_gpu_egnn.py::_sequence)."""
    if step.encoding is not None:
        x = step.encoding(x)
    h_i, h_j = GatherEmbeddingSelection([0, 1])([h, ei])
    m = step.edge_mlp(LazyConcatenate()([h_i, h_j, x]))
    if step.attention_mlp is not None:
        m = LazyMultiply()([step.attention_mlp(m), m])
    return PoolingLocalEdges(pooling_method="sum")([h, m, ei])


def _egnn_inputs(case):
    return (_rag(case["h"], case["row_splits"]), _rag(case["x"], case["index_splits"]),
            _rag(case["indices"], case["index_splits"]))


def _run(fn, h, x, ei, g):
    """(out, h_bar, x_bar) of ``fn(h, x, ei)`` with the upstream gradient ``g``."""
    hv = h.values.detach().clone().requires_grad_(True)
    xv = x.values.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        out = fn(h.with_values(hv), x.with_values(xv), ei).values
        gh, gx = torch.autograd.grad(out, [hv, xv], g)
    return out.detach(), gh, gx


def _check_egnn(name, fused=True, sequence=True):
    case = T.egnn_case(**T.egnn_cases()[name])
    step = _step(case)
    h, x, ei = _egnn_inputs(case)
    g = torch.from_numpy(case["g"]).cuda()
    r32, r64 = T.egnn_restate(case, torch.float32), T.egnn_restate(case, torch.float64)
    runs = []
    if fused:
        runs.append(("fused", _run(step, h, x, ei, g)))
        with torch.no_grad():
            assert torch.equal(step(h, x, ei).values, runs[0][1][0])     # saving the pre-activations changes no bit
    if sequence:
        runs.append(("layer sequence", _run(lambda a, b, c: _sequence(step, a, b, c), h, x, ei, g)))
    for k, part in enumerate(("forward", "h_bar", "x_bar")):
        if r64[k].size == 0:
            assert all(tuple(res[k].shape) == r64[k].shape for _, res in runs)
            continue
        cap = ENC_REV_CAP if part == "x_bar" else 5e-5
        for route, res in runs:
            assert_rows_close(res[k].cpu().numpy(), r32[k], r64[k], what="EGNN %s %s %s" % (name, part, route), cap=cap)
        if len(runs) == 2:
            a, b = runs[0][1][k].cpu().numpy(), runs[1][1][k].cpu().numpy()
            bar = max(1e-5, min(2 * rowwise_rel(r32[k], r64[k]), cap))
            assert rowwise_rel(a, b) <= 2 * bar, "EGNN %s %s: fused vs layer sequence %.3g (bar %.3g)" % (
                name, part, rowwise_rel(a, b), 2 * bar)
    isolated = torch.from_numpy(T.in_degrees(case["flat"], case["rows"]) == 0).cuda()
    assert bool(isolated.any()) or case["rows"] == 5          # every hub batch has receivers without edges
    for _, res in runs:
        assert torch.all(res[0][isolated] == 0)
    return case, step, runs


@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("attention", [True, False])
@pytest.mark.parametrize("encoding", [True, False])
def test_egnn_edge_step_hub_receivers(order, attention, encoding):
    """Rows 1 and 2: receivers of 1 to 1000 edges; one starts on a tile boundary, one ends on one, one covers 30 tiles."""
    _check_egnn("hub-%s-att%d-enc%d" % (order, attention, encoding))


def test_egnn_edge_step_hub_receivers_with_self_loops_and_duplicated_edges():
    _check_egnn("hub-selfdup")


@pytest.mark.parametrize("edges", T.TILE_EXACT_SIZES)
def test_egnn_edge_step_tile_exact_sizes(edges):
    """Row 2: E below one tile, exactly one and two tiles, one over; E = 0 with N = 5 (the finishing pass alone)."""
    case, step, runs = _check_egnn("exact%d" % edges)
    if edges == 0:
        out, gh, gx = runs[0][1]
        assert tuple(out.shape) == (5, 128) and torch.all(out == 0)
        assert tuple(gh.shape) == (5, 128) and torch.all(gh == 0) and tuple(gx.shape) == (0, 1)


@pytest.mark.parametrize("dim_half,interleave", [(1, False), (1, True), (10, False), (10, True), (32, False), (32, True),
                                                 (0, False)])
def test_egnn_edge_step_encoding_widths(dim_half, interleave):
    """Row 3: K = 1 (two columns), the model's 10, K = 32 (C = 64, the widest the kernel takes) and the bare norm."""
    _check_egnn("width%d-il%d" % (dim_half, interleave), sequence=dim_half != 1)


def test_egnn_edge_step_encoding_of_66_columns_takes_the_layer_sequence():
    case = T.egnn_case(**T.egnn_cases()["width33"])
    step = _step(case)
    assert fused_edge_supported(128, step.edge_mlp, step.attention_mlp, step.encoding, "sum") is False
    assert fused_edge_supported(128, step.edge_mlp, step.attention_mlp, PositionEncodingBasisLayer(dim_half=32), "sum")
    _check_egnn("width33", fused=False)


@pytest.mark.parametrize("case", ["act-%s" % a for a in T.HIDDEN_ACTIVATIONS] + ["nobias0", "nobias1", "nobias2"])
def test_egnn_edge_step_activations_and_missing_biases(case):
    """Row 3: every hidden activation code in both layers (pairs in rotation), the gate with sigmoid, tanh and linear;
    each Dense in turn without its bias."""
    kw = T.egnn_cases()[case]
    for act in tuple(kw.get("acts", ())) + (kw.get("gate", "sigmoid"),):
        assert act in _ffi.ACTIVATION_CODES and act in eref.ACTIVATIONS
    _, step, _ = _check_egnn(case)
    if case.startswith("nobias"):
        k = int(case[-1])
        layers = step.edge_mlp.mlp_dense_layer_list + step.attention_mlp.mlp_dense_layer_list
        assert [lay.bias is None for lay in layers] == [i == k for i in range(3)]


def _reordered(case, key):
    """Permutation of the edge list that sorts every graph's edges by ``key(rows)`` (numpy sort keys, stable)."""
    es = case["index_splits"]
    return np.concatenate([es[k] + key(case["indices"][es[k]:es[k + 1]]) for k in range(len(es) - 1)]).astype(np.int64)


def test_egnn_edge_step_hub_receivers_bit_equality():
    """Two runs, a second stream, and a stable reorder by sender (every receiver keeps its list order): the same bits."""
    case = T.egnn_case(**T.egnn_cases()["hub-sorted-att1-enc1"])
    step = _step(case)
    es = case["index_splits"]
    # senders ascending inside every receiver's list, as a molecule's edge list has them
    base = _reordered(case, lambda rows: np.lexsort((rows[:, 1], rows[:, 0])))
    case = dict(case, indices=case["indices"][base], x=case["x"][base])
    h, x, ei = _egnn_inputs(case)
    g = torch.from_numpy(case["g"]).cuda()
    first = _run(step, h, x, ei, g)
    second = _run(step, h, x, ei, g)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        third = _run(step, h, x, ei, g)
    s.synchronize()
    for a, b, c in zip(first, second, third):
        assert torch.equal(a, b) and torch.equal(a, c)
    perm = _reordered(case, lambda rows: np.argsort(rows[:, 1], kind="stable"))
    assert not np.array_equal(perm, np.arange(len(perm)))
    x2, ei2 = _rag(case["x"][perm], es), _rag(case["indices"][perm], es)
    out2, gh2, gx2 = _run(step, h, x2, ei2, g)
    assert torch.equal(out2, first[0]) and torch.equal(gh2, first[1])
    assert torch.equal(gx2, first[2][torch.from_numpy(perm).cuda()])


def test_egnn_model_with_three_tiles_per_receiver():
    from gcnn_keras_amd.literature import EGNN
    b = synth.egnn_batch(**T.EGNN_MODEL_BATCH)
    deg = np.bincount(eref.flat_edges(b)[:, 0], minlength=len(b["node_coordinates"]))
    assert deg.max() == 69 and deg[:70].min() > 64
    m = EGNN.make_model(**synth.EGNN_MD17)
    p = list(synth.egnn_params(m, seed=14).values())
    m.set_weights(p)
    assert m.fused_edge_blocks == [True] * 7
    efm = EnergyForceModel(model_energy=m, coordinate_input=1, output_to_tensor=False, output_squeeze_states=True)
    eng, force = efm([_rag(b["node_attributes"], b["node_splits"]), _rag(b["node_coordinates"], b["node_splits"]),
                      _rag(b["edge_indices"], b["edge_splits"])])
    e64, f64 = eref.energy_forces(p, b, m.config, dtype=torch.float64)
    e32, f32 = eref.energy_forces(p, b, m.config, dtype=torch.float32)
    assert_rows_close(eng.cpu().numpy().reshape(-1, 1), e32.numpy(), e64.numpy(), what="EGNN 70-atom energy")
    assert_forces_close(force.values.cpu().numpy(), f32.numpy(), f64.numpy(), b["node_splits"], what="EGNN 70-atom forces")
    assert np.all(force.values.cpu().numpy()[70] == 0)        # the lone atom


# ====================================================================================================== DimeNet++
def _triplet_block(case):
    e, t, nsbf = case["rows"], len(case["flat"]), case["nsbf"]
    block = DimNetInteractionPPBlock(128, 64, 8, 1, 2)
    block.ensure_built([(None, None, 128), (None, None, 6), (None, None, nsbf), (None, None, 2)])
    block.dense_sbf1.set_weights([case["w1"]])
    block.dense_sbf2.set_weights([case["w2"]])
    down = _rag(case["xdown"], case["row_splits"])
    rbf = _rag(np.zeros((e, 8), np.float32), case["row_splits"])      # the step reads only its row count and splits
    sbf = _rag(case["sbf"], case["index_splits"])
    ai = _rag(case["indices"], case["index_splits"])
    assert t == int(sbf.values.shape[0])
    return block, down, rbf, sbf, ai


def _check_triplet(nsbf, order, fused):
    case = T.triplet_case(nsbf, order, seed=11)
    block, down, rbf, sbf, ai = _triplet_block(case)
    assert bool(block.fused_triplet(nsbf)) is fused
    xv = down.values.detach().clone().requires_grad_(True)
    sv = sbf.values.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        out = block.triplet_step(down.with_values(xv), rbf, sbf.with_values(sv), ai).values
        x_bar, s_bar = torch.autograd.grad(out, [xv, sv], torch.from_numpy(case["g"]).cuda())
    r32, r64 = T.triplet_restate(case, torch.float32), T.triplet_restate(case, torch.float64)
    for k, (name, got) in enumerate((("forward", out), ("xdown_bar", x_bar), ("sbf_bar", s_bar))):
        assert_rows_close(got.detach().cpu().numpy(), r32[k], r64[k],
                          what="triplet step nsbf=%d %s %s" % (nsbf, order, name))
    none = torch.from_numpy(T.in_degrees(case["flat"], case["rows"]) == 0).cuda()
    assert bool(none.any()) and torch.all(out.detach()[none] == 0)           # edges without triplets
    if fused:
        with torch.no_grad():
            block.use_fused_triplet = False
            seq = block.triplet_step(down, rbf, sbf, ai).values
            block.use_fused_triplet = True
        assert_rows_close(seq.cpu().numpy(), r32[0], r64[0], what="triplet layer sequence nsbf=%d %s" % (nsbf, order))


@pytest.mark.parametrize("nsbf", T.TRIPLET_WIDTHS)
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_triplet_step_hub_edges(nsbf, order):
    """Rows 4 and 5: basis widths 1, 7, 42 and 64 (the widest); 0 to 1000 triplets per receiving edge."""
    _check_triplet(nsbf, order, fused=True)


def test_triplet_step_basis_of_65_columns_takes_the_layer_sequence():
    _check_triplet(65, "sorted", fused=False)


def _angle_and_basis_rows(b):
    """[(name, engine rows, float32 rows, float64 rows, cap)] of EdgeAngle, its reverse, the 7 x 6 spherical basis and its
    reverse on a DimeNet++ batch."""
    x = _rag(b["node_coordinates"], b["node_splits"])
    ei, ai = _rag(b["edge_indices"], b["edge_splits"]), _rag(b["angle_indices"], b["angle_splits"])
    p1, p2 = NodePosition()([x, ei])
    v, d = LazySubtract()([p1, p2]), NodeDistanceEuclidean()([p1, p2])
    ei_flat, ai_flat = (torch.from_numpy(a) for a in dref.flat_indices(b))
    assert int(np.bincount(ai_flat[:, 0].numpy()).max()) == 70
    # the angle and its reverse
    vv = v.values.detach().clone().requires_grad_(True)
    g = torch.from_numpy(np.random.default_rng(3).normal(size=(len(ai_flat), 1)).astype(np.float32)).cuda()
    with torch.enable_grad():
        th = EdgeAngle()([v.with_values(vv), ai]).values
        (v_bar,) = torch.autograd.grad(th, [vv], g.reshape(th.shape))
    layer = SphericalBasisLayer(7, 6, 5.0)
    dv = d.values.detach().clone().requires_grad_(True)
    tv = th.detach().clone().requires_grad_(True)
    theta = ai.with_values(tv)
    with torch.enable_grad():
        sbf = layer([d.with_values(dv), theta, ai]).values
        gs = torch.from_numpy(np.random.default_rng(1).normal(size=tuple(sbf.shape)).astype(np.float32)).cuda()
        d_bar, t_bar = torch.autograd.grad(sbf, [dv, tv], gs)
    outs = {}
    for dt in (torch.float32, torch.float64):
        xr = torch.tensor(b["node_coordinates"], dtype=dt)
        rv = (xr[ei_flat[:, 0]] - xr[ei_flat[:, 1]]).detach().requires_grad_(True)
        t = dref.vector_angle(rv[ai_flat[:, 0]], rv[ai_flat[:, 1]])
        (gv,) = torch.autograd.grad(t, [rv], g.cpu().to(dt).reshape(-1))
        rd = torch.linalg.norm(rv.detach(), dim=-1).requires_grad_(True)
        t2 = t.detach().requires_grad_(True)
        s = dref.spherical_basis(rd, t2, ai_flat[:, 1], layer, dt)
        gd, gt = torch.autograd.grad(s, [rd, t2], gs.cpu().to(dt))
        outs[dt] = (t.detach().numpy()[:, None], gv.numpy(), s.detach().numpy(), gd.numpy()[:, None], gt.numpy()[:, None])
    r32, r64 = outs[torch.float32], outs[torch.float64]
    rows = [("edge angle", th.detach().reshape(-1, 1), 0, 5e-5), ("edge angle reverse", v_bar, 1, 5e-5),
            ("sbf forward", sbf.detach(), 2, SBF_CAP), ("sbf d_bar", d_bar, 3, SBF_CAP), ("sbf theta_bar", t_bar, 4, SBF_CAP)]
    return [(name, got.cpu().numpy().reshape(len(got), -1), r32[k], r64[k], cap) for name, got, k, cap in rows]


@pytest.mark.parametrize("shuffled", [False, True])
def test_edge_angle_and_basis_reverse_with_many_triplets_per_edge(shuffled):
    """Row 5: a 72-atom all-connected molecule, 70 triplets on every edge (the lane-strided loops run twice)."""
    for name, got, r32, r64, cap in _angle_and_basis_rows(T.many_triplets_batch(shuffled)):
        assert_rows_close(got, r32, r64, what="72 atoms%s %s" % (" shuffled" if shuffled else "", name), cap=cap)


# ====================================================================================================== ACSF
def _acsf_layer(name, kind, table, mult):
    elements = list(T.acsf_elements(name))
    if kind == "g2":
        return ACSFG2(eta_rs_rc=table, element_mapping=elements)
    return ACSFG4(eta_zeta_lambda_rc=table, element_mapping=elements, multiplicity=mult)


def _check_acsf(name):
    kind, b, table, mult, with_jvp = T.acsf_cases()[name]
    layer = _acsf_layer(name, kind, table, mult)
    width = layer.num_relations * layer.num_functions
    g, h = T.acsf_upstream(name, b, width)
    z = _rag(b["node_number"], b["node_splits"])
    idx = _rag(b["angle_indices"], b["angle_splits"]) if kind == "g4" else _rag(b["edge_indices"], b["edge_splits"])
    xd = torch.as_tensor(b["node_coordinates"]).cuda().requires_grad_(True)
    gd = torch.from_numpy(g).cuda().requires_grad_(True)
    out = layer([z, RaggedTensor(xd, torch.as_tensor(b["node_splits"]).cuda()), idx]).values
    dx, = torch.autograd.grad(out, xd, grad_outputs=gd, create_graph=with_jvp)
    got = [out.detach(), dx.detach()]
    if with_jvp:
        from gcnn_keras_amd.autograd import coordinate_hessian_discarded
        with coordinate_hessian_discarded():
            gbar, = torch.autograd.grad(dx, gd, grad_outputs=torch.from_numpy(h).cuda())
        got.append(gbar)
    r32, r64 = (T.acsf_restate(kind, b, table, dt, T.acsf_elements(name), mult, h if with_jvp else None, g)
                for dt in (torch.float32, torch.float64))
    for k, part in enumerate(("forward", "reverse dx", "jvp g_bar")[:len(got)]):
        assert_rows_close(got[k].cpu().numpy(), r32[k], r64[k], what="ACSF %s %s" % (name, part))
    return layer, b


@pytest.mark.parametrize("kind", ["g2", "g4"])
@pytest.mark.parametrize("table", ["plain", "target"])
def test_acsf_wide_tables_with_a_cutoff_per_function(kind, table):
    """Rows 6 and 7: 70 (G2) and 100 (G4) functions per relation, each with its own cutoff; empty graphs in the batch."""
    _check_acsf("wide-%s-%s" % (kind, table))


@pytest.mark.parametrize("case", ["many-g2-150", "many-g2-64-65", "many-g4-40"])
def test_acsf_many_neighbours(case):
    """Row 8: 149 pairs per receiver, receivers of exactly 64 and 65 pairs, 1482 triplets per receiver."""
    _check_acsf(case)


def test_acsf_width_bound():
    """Row 8: R*m = 2048 runs; 4 x 513 is refused; a plain table of 2052 floats is read through the global pointer."""
    _check_acsf("bound-g2-4x512")
    _check_acsf("global-g2-4x171")
    _, b, _, _, _ = T.acsf_cases()["bound-g2-4x512"]
    layer = ACSFG2(eta_rs_rc=T.g2_table(4, 513, 52), element_mapping=[1, 6, 7, 8])
    with pytest.raises(ValueError, match="exceeds 2048"):
        layer([_rag(b["node_number"], b["node_splits"]), _rag(b["node_coordinates"], b["node_splits"]),
               _rag(b["edge_indices"], b["edge_splits"])])


# ====================================================================================================== one large graph
def test_painn_on_a_graph_of_5000_points_takes_the_gather_kernels():
    """Row 9: more than 4096 nodes in one graph - no LDS tile table, the gather kernels serve forward and reverse."""
    from gcnn_keras_amd.literature import PAiNN
    from oracle import torch_force_oracle as tfo
    b = T.large_graph_batch()
    p = synth.painn_params(seed=8, random_bias=True)
    energy = PAiNN.make_model(equiv_initialize_kwargs={"dim": 3, "method": "eps"})
    energy.set_weights(painn_weight_list(p))
    assert energy.fused is not None
    model = EnergyForceModel(model_energy=energy, coordinate_input=1, energy_output=0, output_to_tensor=False,
                             output_squeeze_states=True)
    x = mol_inputs(b)
    out = model(x)
    eng, force = out["energy"].cpu().numpy(), out["force"].values.cpu().numpy()
    assert energy.fused.slot_of(x, grad=True).tiles0 is None and energy.fused.slot_of(x, grad=True).tiles1 is None
    (e32, f32), (e64, f64) = (tfo.painn_energy_force(p, b, dt, equiv_method="eps", cutoff=None)
                              for dt in (torch.float32, torch.float64))
    assert eng.shape == (1, 1) and force.shape == (5000, 3)
    assert_rows_close(eng, np.asarray(e32).reshape(1, 1), np.asarray(e64).reshape(1, 1), what="PaiNN 5000 points energy")
    assert_forces_close(force, f32, f64, b["node_splits"], what="PaiNN 5000 points forces")
    fwd = energy(mol_inputs(b))
    assert_rows_close(fwd.cpu().numpy(), np.asarray(e32).reshape(1, 1), np.asarray(e64).reshape(1, 1),
                      what="PaiNN 5000 points forward")
    energy.fused.check_flags()


def test_schnet_on_a_graph_of_5000_points():
    from gcnn_keras_amd.literature import Schnet
    from oracle import kgcnn_oracle as ko
    b = T.large_graph_batch()
    p = synth.schnet_params(seed=7, random_bias=True)
    model = Schnet.make_model(depth=3)
    model.set_weights(list(p.values()))
    got = model(mol_inputs(b)).cpu().numpy()
    refs = [ko.schnet_forward(ko.to_dtype(p, dt), ko.R(b["node_number"], b["node_splits"]),
                              ko.R(b["node_coordinates"].astype(dt), b["node_splits"]),
                              ko.R(b["edge_indices"], b["edge_splits"]), depth=3) for dt in (np.float32, np.float64)]
    assert_rows_close(got, refs[0], refs[1], what="SchNet 5000 points")
