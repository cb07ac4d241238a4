"""The kernels of the fused SchNet energy + force pass (csrc/mp_schnet_bwd.hip: ``mp_schnet_force_launch``) off the
molecular shapes, kernel by kernel through the C ABI against the float64 restatements of tests/schnet_force_cases.py, and
one composed run: the FP32-MFMA build of the distance gradient (32 bins), its tile, workgroup and second-trip edges, the
second lane round and the second node trip of the force kernel, the SAVE builds of the node chains at their tile edges and
on their second trip, the readout's 8-row rounds, 24-row prefetch and second graph trip.  Every output buffer is filled
with NaN and carries a tail behind its logical end that must still be NaN afterwards; every case compares once.

Bars (none of its own): 2e-5 of the tensor's largest magnitude for the chains, the saved derivatives and ``g_d``
(``_close`` of tests/test_gpu_schnet_bwd.py), 1e-5 of the largest force for mp_schnet_force_from_gd_f32 (the force test
there), the defaults of ``parity.assert_rows_close`` / ``assert_forces_close`` with the float64 twin for the readout and
the composed run.

Distance of the float32 restatement from its float64 twin on these cases, in the metric of the comparison (NumPy, CPU;
asserted at or below half the bar by tests/test_schnet_force_cases.py, which prints each figure):

  g_d, 40 nodes / 1300 edges, bins 1 2 30 31 32, no bias (20, 32)      2.0e-07..5.7e-07
  g_d, exact M = 1 31 32 33 127 128 129 (5 nodes), 9 x 128 edges       1.1e-07..3.1e-07
  g_d, 32 801 edges over 40 nodes, bins 20 / 32                        2.9e-07 / 2.6e-07
  g_d, hubs 31 1 32 33 7 64 65 100 1000 (sorted, shuffled, self loops) 4.2e-07
  g_d, d = 0, d = 3 x distance, offset 0.75, sigma 0.1, clamped ids    2.2e-07..3.1e-07; |pre1| up to 100: 3.6e-07
  forces from g_d, hubs on the receiver / sender side, shuffled        2.1e-07 / 1.1e-06 / 6.1e-07; self loops 3.5e-07
  forces from g_d, ring over 8209 nodes                                8.1e-08
  node chains n x d2 dl0 dl1 h, N = 1 15 16 17 8193, with / no biases  8.2e-08..6.7e-07; pre-activations +-30: <= 1.7e-06
  readout out / g_pool rows, sizes 0 1 7 8 9 23 24 25 33 100 0 16 0    <= 1.5e-06 / 1.5e-07; linear head 9.9e-08
  readout out / g_pool rows, 4101 graphs of 0..2 rows                  <= 2.1e-06 / 5.4e-07; linear head 1.6e-07
  model, 70 + 1 + 0 + 21 atoms, cutoff 8 A, bins 32 / 25               energy 7.8e-07 (shuffled 2.7e-06) / 3.3e-07,
                                                                       forces <= 1.8e-06 of a molecule's scale
"""
import numpy as np
import pytest
import torch

import schnet_force_cases as C
from gcnn_keras_amd import _ffi, synth
from gcnn_keras_amd.ragged import RaggedTensor
from helpers import mol_inputs
from oracle import torch_force_oracle as tfo
from parity import assert_forces_close, assert_rows_close

pytestmark = pytest.mark.gpu

TAIL = 5      # elements / rows behind the logical end of every output buffer


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan(rows, *inner):
    return torch.full((rows + TAIL,) + inner, float("nan"), dtype=torch.float32, device="cuda")


def _held(a, rows, value=7.0):
    """Device copy of ``a`` (rows, ...) with TAIL rows of ``value`` behind it: an input the kernel updates in place."""
    tail = np.full((TAIL,) + a.shape[1:], value, np.float32)
    return _dev(np.concatenate([a.astype(np.float32), tail], axis=0))


def _tail_is_nan(buf, rows, what):
    assert bool(torch.isnan(buf[rows:]).all()), "%s: a store past row %d" % (what, rows)


def _close(got, want, bar, what):
    """``_close`` of tests/test_gpu_schnet_bwd.py: every element written and finite, the largest error at most ``bar`` of
    the reference's largest magnitude (printed first)."""
    got = got.detach().double().cpu().numpy()
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.all(np.isfinite(got)), "%s: %d elements unwritten or not finite" % (what, int(np.sum(~np.isfinite(got))))
    err = C.max_rel(got, want)
    print("[edges] %s: %.2e of the largest magnitude from float64 (bar %.0e)" % (what, err, bar))
    assert err <= bar, "%s: off by %.3g of the largest magnitude %.3g (bar %.1g)" % (what, err, np.abs(want).max(), bar)


# ------------------------------------------------------------------------------------- A. distance gradient of cfconv
def _bwd_image(c, bins=None):
    image = torch.empty(_ffi.lib().mp_cfconv_bwd_packed_floats(), dtype=torch.float32, device="cuda")
    w1, b1, w2 = _dev(c["w1"]), _dev(c["b1"]), _dev(c["w2"])
    _ffi.call("mp_cfconv_bwd_pack_f32", _ffi.ptr(w1), _ffi.ptr(b1), c["bins"] if bins is None else bins, _ffi.ptr(w2),
              _ffi.ptr(image), _ffi.stream())
    torch.cuda.synchronize()
    return image


def _dist_grad(c, t, image, g_d, accumulate=0, m=None, n=None, bins=None):
    _ffi.call("mp_cfconv_gauss_dist_grad_f32", _ffi.ptr(t["x"]), _ffi.ptr(t["g_out"]), c["N"] if n is None else n,
              _ffi.ptr(t["dist"]), c["bins"] if bins is None else bins, c["distance"], c["sigma"], c["offset"],
              _ffi.ptr(image), _ffi.ptr(t["recv"]), _ffi.ptr(t["send"]), c["M"] if m is None else m, accumulate,
              _ffi.ptr(g_d), _ffi.stream())
    torch.cuda.synchronize()


def _operands(c):
    return {k: _dev(c[k]) for k in ("x", "g_out", "dist", "recv", "send")}


@pytest.mark.parametrize("name", sorted(set(C.dist_grad_cases()) - {"accumulate"}))
def test_distance_gradient(name):
    """g_d of every case against the float64 restatement: both builds of the basis GEMMs, absent b1, edge counts around
    the tile and the workgroup, the second trip, hubs with self loops (d = 0) and duplicates, distances at 0 and far
    outside the basis, an offset, a narrow basis, saturated pre-activations, clamped node ids."""
    c = C.dist_grad_case(**C.dist_grad_cases()[name])
    g_d = _nan(c["M"])
    _dist_grad(c, _operands(c), _bwd_image(c), g_d)
    _close(g_d[:c["M"]], C.dist_grad_restate(c, np.float64), C.BAR_CHAIN, "g_d " + name)
    _tail_is_nan(g_d, c["M"], name)


def test_distance_gradient_accumulate_adds_the_same_value_bit_for_bit():
    c = C.dist_grad_case(**C.dist_grad_cases()["accumulate"])
    t, image, m = _operands(c), _bwd_image(c), c["M"]
    g_d = _nan(m)
    _dist_grad(c, t, image, g_d, accumulate=0)
    first = g_d.clone()
    assert bool(torch.isfinite(first[:m]).all()) and bool(torch.isnan(first[m:]).all())     # exactly the first M entries
    _close(first[:m], C.dist_grad_restate(c, np.float64), C.BAR_CHAIN, "g_d written")
    _dist_grad(c, t, image, g_d, accumulate=1)
    assert torch.equal(g_d[:m], first[:m] + first[:m])
    _tail_is_nan(g_d, m, "accumulate")


def test_distance_gradient_empty_launches_and_basis_bounds():
    c = C.dist_grad_case(**C.dist_grad_cases()["exact33"])
    t, image = _operands(c), _bwd_image(c)
    g_d = _nan(c["M"])
    _dist_grad(c, t, image, g_d, m=0)
    _dist_grad(c, t, image, g_d, n=0)
    assert bool(torch.isnan(g_d).all())                   # MP_OK and nothing touched
    for bins in (0, 33):
        with pytest.raises(ValueError):
            _bwd_image(c, bins=bins)
        with pytest.raises(ValueError):
            _dist_grad(c, t, image, g_d, bins=bins)
    assert bool(torch.isnan(g_d).all())


# ------------------------------------------------------------------------------------- B. forces from dE/dd
@pytest.mark.parametrize("name", sorted(C.force_cases()))
def test_force_from_distance_gradient(name):
    """mp_schnet_force_from_gd_f32 alone (``g_d`` is a given random vector): degrees 64, 65, 100 and 1000 on either
    column with and without its permutation, 8209 nodes (second node trip) most of which are isolated, coincident pairs
    and self loops (d = 0), both signs of ``scale``, no edges at all."""
    c = C.force_case(**C.force_cases()[name])
    n, m = c["N"], c["M"]
    if m:
        node = RaggedTensor.from_numpy(c["xyz"], np.array([0, n], np.int64))
        plan = RaggedTensor.from_numpy(c["edges"], np.array([0, m], np.int64)).index_plan(node)
        ptr0, perm0, _ = plan.csr(0)
        ptr1, perm1, _ = plan.csr(1)
        sorted0, sorted1 = (bool(np.all(np.diff(c["edges"][:, k]) >= 0)) for k in (0, 1))
        assert (perm0 is None) == sorted0 and (perm1 is None) == sorted1
    else:       # the CSR of no edges
        ptr0, ptr1 = (torch.zeros(n + 1, dtype=torch.int32, device="cuda") for _ in range(2))
        perm0 = perm1 = None
    t = [_dev(c[k]) if m else None for k in ("g_d", "xyz", "dist", "recv", "send")]
    t[1] = _dev(c["xyz"])
    out = _nan(n, 3)
    _ffi.call("mp_schnet_force_from_gd_f32", *[_ffi.ptr(v) for v in t], _ffi.ptr(ptr0), _ffi.ptr(perm0), _ffi.ptr(ptr1),
              _ffi.ptr(perm1), n, m, c["scale"], _ffi.ptr(out), _ffi.stream())
    torch.cuda.synchronize()
    _tail_is_nan(out, n, name)
    got = out[:n].cpu().numpy()
    touched = np.zeros(n, bool)
    touched[c["edges"].reshape(-1)] = True
    assert np.all(got[~touched] == 0) and np.all(np.isfinite(got))          # isolated nodes: exact zeros
    if m:
        _close(out[:n], C.force_restate(c, np.float64), C.BAR_FORCE, "forces " + name)
    else:
        assert not got.any()


# ------------------------------------------------------------------------------------- C. SAVE builds of the node chains
def _pack(w):
    """mp_schnet_node_pack_f32 image of a (K, U) matrix."""
    w = _dev(w)
    out = torch.empty(w.numel(), dtype=torch.float32, device="cuda")
    _ffi.call("mp_schnet_node_pack_f32", _ffi.ptr(w), int(w.shape[0]), int(w.shape[1]), _ffi.ptr(out), _ffi.stream())
    torch.cuda.synchronize()
    return out


def _mid(c, img, bias, bufs, flags, d2="d2"):
    _ffi.call("mp_schnet_node_update_save_f32", _ffi.ptr(bufs["agg"]), c["N"], _ffi.ptr(img["W2"]), _ffi.ptr(bias["b2"]),
              _ffi.ptr(img["W3"]), _ffi.ptr(bias["b3"]), _ffi.ptr(bufs["n"]), _ffi.ptr(img["Wx"]), _ffi.ptr(bufs["x"]),
              _ffi.ptr(bufs.get(d2)), flags, _ffi.stream())
    torch.cuda.synchronize()


def _last(c, img, bias, bufs, flags, saved=("d2", "dl0", "dl1")):
    _ffi.call("mp_schnet_node_last_save_f32", _ffi.ptr(bufs["agg"]), c["N"], _ffi.ptr(img["W2"]), _ffi.ptr(bias["b2"]),
              _ffi.ptr(img["W3"]), _ffi.ptr(bias["b3"]), _ffi.ptr(bufs["n"]), _ffi.ptr(img["Wl0"]), _ffi.ptr(bias["bl0"]),
              _ffi.ptr(img["Wl1"]), _ffi.ptr(bias["bl1"]), _ffi.ptr(bufs["h"]),
              *[_ffi.ptr(bufs[k]) if k in saved else None for k in ("d2", "dl0", "dl1")], flags, _ffi.stream())
    torch.cuda.synchronize()


def _node_buffers(c):
    n = c["N"]
    return {"agg": _held(c["agg"], n), "n": _held(c["n"], n), "x": _nan(n, C.F), "d2": _nan(n, C.F), "dl0": _nan(n, C.F),
            "dl1": _nan(n, C.H), "h": _nan(n, C.H)}


def _node_setup(c):
    img = {k: _pack(c[k]) for k in ("W2", "W3", "Wx", "Wl0", "Wl1")}
    bias = {k: _dev(c[k]) for k in ("b2", "b3", "bl0", "bl1")}
    return img, bias


NODE_RUNS = [(n, True, False) for n in C.NODE_COUNTS] + [(17, False, False), (8193, False, False), (37, True, True)]


@pytest.mark.parametrize("flags", [2, 3])
@pytest.mark.parametrize("n,bias,saturated", NODE_RUNS)
def test_node_chain_save_builds(n, bias, saturated, flags):
    """mp_schnet_node_update_save_f32 (MID) and mp_schnet_node_last_save_f32 (LAST) with exact (2) and fast (3) softplus:
    node counts around the 16-node tile and one past the 512 persistent tiles, every bias absent, pre-activations out to
    +-30.  MID: ``n`` in place, ``x`` and ``d2``; LAST: ``h``, ``d2``, ``dl0``, ``dl1``; the consumed ``agg`` rows are zero
    afterwards and nothing behind row N is touched."""
    c = C.node_case(n, bias=bias, saturated=saturated)
    img, b = _node_setup(c)
    want = C.node_restate(c, np.float64)
    tag = "N=%d flags=%d%s%s" % (n, flags, "" if bias else " no bias", " saturated" if saturated else "")
    for chain, run, outputs in (("MID", _mid, C.MID_OUTPUTS), ("LAST", _last, C.LAST_OUTPUTS)):
        bufs = _node_buffers(c)
        run(c, img, b, bufs, flags)
        for k in outputs:
            _close(bufs[k][:n], want[k], C.BAR_CHAIN, "%s %s %s" % (chain, tag, k))
            if k != "n":
                _tail_is_nan(bufs[k], n, "%s %s %s" % (chain, tag, k))
            if k in ("d2", "dl0", "dl1"):          # saved sigmoids stay inside [0, 1]
                assert float(bufs[k][:n].min()) >= 0.0 and float(bufs[k][:n].max()) <= 1.0, (chain, tag, k)
        assert not bool(bufs["agg"][:n].any()), "%s %s: consumed agg rows are zero again" % (chain, tag)
        assert bool((bufs["agg"][n:] == 7.0).all()) and bool((bufs["n"][n:] == 7.0).all()), (chain, tag)
        if chain == "MID":
            assert bool(torch.isnan(bufs["h"]).all()) and bool(torch.isnan(bufs["dl0"]).all())
        else:                                      # LAST reads the node state only
            assert torch.equal(bufs["n"][:n], _dev(c["n"])) and bool(torch.isnan(bufs["x"]).all())


def test_node_chain_save_builds_refuse_partial_buffers_and_unpacked_weights():
    c = C.node_case(17)
    img, b = _node_setup(c)
    bufs = _node_buffers(c)
    with pytest.raises(ValueError):
        _last(c, img, b, bufs, 2, saved=("d2", "dl0"))                # two of the three derivative buffers
    with pytest.raises(ValueError):
        _last(c, img, b, bufs, 2, saved=("dl1",))
    with pytest.raises(ValueError):
        _last(c, img, b, bufs, 0)                                     # saving without packed images (flag bit 1)
    with pytest.raises(ValueError):
        _mid(c, img, b, bufs, 1)
    for k in ("x", "d2", "dl0", "dl1", "h"):
        assert bool(torch.isnan(bufs[k]).all()), k                    # refused before any launch
    assert torch.equal(bufs["agg"][:17], _dev(c["agg"]))


# ------------------------------------------------------------------------------------- D. readout and dE/dpooled
def _readout(c, head, with_g_pool=True):
    h = _dev(c["h"]) if c["N"] else torch.zeros((1, C.H), device="cuda")
    t = {k: _dev(c[k]) for k in ("splits", "Wo0", "bo0", "Wo1", "bo1")}
    out, g_pool = _nan(c["G"]), _nan(c["G"], C.H)
    linear = head == "linear"
    _ffi.call("mp_schnet_readout_grad_f32", _ffi.ptr(h), _ffi.ptr(t["splits"]), c["G"],
              None if linear else _ffi.ptr(t["Wo0"]), None if linear else _ffi.ptr(t["bo0"]), _ffi.ptr(t["Wo1"]),
              _ffi.ptr(t["bo1"]), _ffi.ptr(out), _ffi.ptr(g_pool) if with_g_pool else None, _ffi.stream())
    torch.cuda.synchronize()
    return out, g_pool


@pytest.mark.parametrize("sizes", ["edges", "trip"])
@pytest.mark.parametrize("bias", [(True, True), (False, True), (True, False)])
def test_readout_and_pooled_gradient(sizes, bias):
    """mp_schnet_readout_grad_f32 on graphs of 0 1 7 8 9 23 24 25 33 100 0 16 0 rows (the 8-row rounds, the three
    prefetched rounds, empty graphs first, inside and last) and on 4101 graphs of 0 to 2 rows (second graph trip): the
    energies and dE/dpooled of the MLP head, the energies of the linear head, with ``bo0`` / ``bo1`` absent."""
    c = C.readout_case(C.READOUT_SIZES if sizes == "edges" else C.readout_trip_sizes(), bias=bias)
    g = c["G"]
    tag = "%s bo0=%d bo1=%d" % (sizes, bias[0], bias[1])
    (o32, g32), (o64, g64) = (C.readout_restate(c, dt) for dt in (np.float32, np.float64))
    out, g_pool = _readout(c, "mlp")
    for buf, what in ((out, "out"), (g_pool, "g_pool")):
        _tail_is_nan(buf, g, what)
        assert bool(torch.isfinite(buf[:g]).all()), "readout %s %s: unwritten or not finite" % (tag, what)
    assert_rows_close(out[:g].cpu().numpy().reshape(-1, 1), o32, o64, what="readout MLP head %s out" % tag)
    assert_rows_close(g_pool[:g].cpu().numpy(), g32, g64, what="readout MLP head %s g_pool" % tag)
    (l32, _), (l64, _) = (C.readout_restate(c, dt, head="linear") for dt in (np.float32, np.float64))
    out, g_pool = _readout(c, "linear", with_g_pool=False)
    _tail_is_nan(out, g, "linear out")
    assert bool(torch.isnan(g_pool).all())
    got = out[:g].cpu().numpy().reshape(-1, 1)
    assert np.all(np.isfinite(got)) and np.all(got[c["sizes"] == 0] == 0)       # an empty graph's energy is 0
    assert_rows_close(got, l32, l64, what="readout linear head %s out" % tag)


def test_readout_refuses_a_pooled_gradient_for_the_linear_head():
    c = C.readout_case()
    with pytest.raises(ValueError):
        _readout(c, "linear", with_g_pool=True)


# ------------------------------------------------------------------------------------- E. composed
@pytest.mark.parametrize("bins,shuffled", [(32, False), (32, True), (25, False)])
def test_schnet_fused_force_pass_on_a_molecule_with_more_than_64_neighbours(bins, shuffled):
    """``Schnet.make_model(depth=3)`` under ``EnergyForceModel`` on the fused route (eager first, the captured graph
    afterwards) on graphs of 70, 1, 0 and 21 atoms inside an 8 A cutoff - every atom of the first has more than 64
    neighbours on both columns - with 32 (FP32-MFMA distance gradient) and 25 bins, edges sorted and shuffled inside
    each graph; energies and forces against the float32 and float64 references, the tape + layer path to the same."""
    from gcnn_keras_amd.literature import Schnet
    from gcnn_keras_amd.model.force import EnergyForceModel
    b = C.model_batch(synth.radius_graph, shuffled=shuffled)
    ga = C.MODEL_GAUSS[bins]
    p = synth.schnet_params(seed=7, bins=bins, random_bias=True)
    energy = Schnet.make_model(depth=3, gauss_args=dict(ga))
    energy.set_weights(list(p.values()))
    model = EnergyForceModel(model_energy=energy, coordinate_input=1, energy_output=0, output_to_tensor=False,
                             output_squeeze_states=True)
    inputs = mol_inputs(b)
    first = model(inputs)
    assert energy.fused.last == "eager"
    second = model(inputs)
    assert energy.fused.last == "graph"
    (e32, f32), (e64, f64) = (tfo.schnet_energy_force(p, b, dt, depth=3, gauss_args=ga)
                              for dt in (torch.float32, torch.float64))
    ns = b["node_splits"]
    model.fused = False
    tape = model(inputs)
    # (no bit equality between the two fused calls: a receiver of 69 edges spans three tiles of the forward cfconv kernel,
    # whose boundary partial sums are float atomics - csrc/mp_cfconv.hip - so the order of the adds is free)
    for route, o in (("fused, eager", first), ("fused, graph", second), ("tape", tape)):
        tag = "SchNet 70-atom batch, bins %d %s (%s)" % (bins, "shuffled" if shuffled else "sorted", route)
        eng, force = o["energy"].cpu().numpy(), o["force"].values.cpu().numpy()
        assert eng.shape == (4, 1) and force.shape == (int(ns[-1]), 3)
        assert_rows_close(eng, e32, e64, what=tag + " energy")
        assert_forces_close(force, f32, f64, ns, what=tag + " forces")
        assert np.all(force[70] == 0)                                          # the lone atom
