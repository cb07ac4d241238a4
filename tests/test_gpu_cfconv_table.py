"""The cfconv filter table on the GPU (csrc/mp_cfconv.hip: ``cfconv_filter_table_kernel``, ``cfconv_filter_check_kernel``,
``cfconv_table_kernel``) through the C ABI, and the route that uses it (fused.py).

* table rows against the float64 filter at the knots (tests/filter_table_model.py), the self-check words;
* the kernel against the NumPy restatement of the cfconv (tests/cfconv_cases.py, float32 and float64 twins,
  ``parity.assert_rows_close`` at its defaults) on graphs of 5..40 nodes: edge counts around the tile, a receiver over three
  tiles, segments that begin and end on tile and half-tile edges, receivers without edges, an unsorted list through
  ``perm``, the deterministic mode, distances at the ends of the table's domain and far beyond, three basis sizes, an
  offset, every workgroup size;
* the table kernel and the MFMA kernel on the same inputs;
* the route: lone forward against launch-group members, direct launch against replay, ``MPENGINE_FILTER_TABLE=0`` in a
  child process, a weight update that makes the route fall back and one that brings the table back.

Table kernel against the MFMA kernel, the bound: either filter element is within E (MFMA, measured 3.4e-7) resp. the bar
2 E (table) of the float64 filter, in units of the filter's scale S = max |filter|; the issue asks for agreement within the
bar.  A row of the output sums x[send] * filter over the receiver's edges, so the row scale is S * sum_e |x[send_e]|_inf."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cfconv_cases as C
import filter_table_model as M
import topologies as T
from gcnn_keras_amd import _ffi, synth
from gcnn_keras_amd.fused import FILTER_TABLE_BAR, FILTER_TABLE_LOG2_INV_H
from helpers import mol_inputs
from oracle import kgcnn_oracle as ko
from parity import assert_rows_close, rowwise_rel

pytestmark = pytest.mark.gpu

TAIL = 5
F = C.F
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()


def _case(n, edges, bins=20, distance=4.0, sigma=0.4, offset=0.0, seed=0, shuffled=False):
    """Operands in the form of ``cfconv_cases.case`` for a given graph."""
    rng = np.random.default_rng(23000 + 17 * seed + bins)
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    if shuffled:
        e = e[rng.permutation(len(e))]
    xyz = T.points(rng, n, 1.2, min_distance=0.3)
    recv, send = e[:, 0].astype(np.int32), e[:, 1].astype(np.int32)
    return {"N": n, "M": len(e), "bins": bins, "distance": float(f32(distance)), "sigma": float(f32(sigma)),
            "offset": float(f32(offset)), "recv": recv, "send": send,
            "dist": np.linalg.norm(xyz[recv] - xyz[send], axis=1).astype(f32),
            "w1": (rng.standard_normal((bins, F)) * 0.3).astype(f32), "b1": (rng.standard_normal(F) * 0.1).astype(f32),
            "w2": (rng.standard_normal((F, F)) * 0.1).astype(f32), "b2": (rng.standard_normal(F) * 0.1).astype(f32),
            "x": rng.standard_normal((n, F)).astype(f32)}


def _layout(c):
    lay = _ffi.FilterTableLayout()
    _ffi.call("mp_cfconv_filter_table_layout", c["bins"], c["distance"], c["sigma"], c["offset"], FILTER_TABLE_LOG2_INV_H,
              ctypes.byref(lay))
    return lay


def _table(c):
    """(layout, table tensor (rows, 128), error over scale from the self-check words)."""
    lay = _layout(c)
    table = torch.full((lay.rows, F), float("nan"), dtype=torch.float32, device="cuda")
    check = torch.full((2,), float("nan"), dtype=torch.float32, device="cuda")
    w = [_dev(c[k]) for k in ("w1", "b1", "w2", "b2")]
    _ffi.call("mp_cfconv_filter_table_f32", _ffi.ptr(w[0]), _ffi.ptr(w[1]), c["bins"], _ffi.ptr(w[2]), _ffi.ptr(w[3]),
              c["distance"], c["sigma"], c["offset"], ctypes.byref(lay), _ffi.ptr(table), _ffi.ptr(check), _ffi.stream())
    torch.cuda.synchronize()
    err, scale = (float(v) for v in check.cpu().numpy())
    return lay, table, err / scale


def _run(c, flags=0, waves=0, tab=None):
    """One call of mp_cfconv_table_f32 on a fresh ``out`` (N zero rows, NaN rows behind them that must stay NaN)."""
    lay, table, err = tab if tab is not None else _table(c)
    assert err <= FILTER_TABLE_BAR, "the case's table misses its self-check: %.3g" % err
    recv_sorted, perm = C.kernel_order(c)
    t = {k: _dev(v) for k, v in (("x", c["x"]), ("dist", c["dist"]), ("recv", recv_sorted), ("send", c["send"]),
                                 ("perm", perm))}
    n, m = c["N"], c["M"]
    out = torch.full((n + TAIL, F), float("nan"), dtype=torch.float32, device="cuda")
    out[:n] = 0.0
    ws, nbytes = None, 0
    if flags & 32:
        nbytes = _ffi.workspace_bytes("mp_cfconv_det_workspace_bytes", m)
        ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    _ffi.call("mp_cfconv_table_f32", _ffi.ptr(t["x"]), n, _ffi.ptr(t["dist"]), c["offset"], _ffi.ptr(table),
              ctypes.byref(lay), _ffi.ptr(t["recv"]), _ffi.ptr(t["send"]), _ffi.ptr(t["perm"]), m, flags, waves,
              _ffi.ptr(out), _ffi.ptr(ws), nbytes, _ffi.stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[n:]).all()), "a store past row %d" % n
    return out[:n]


def _compare(c, got, what):
    r32, r64 = (C.cfconv_restate(c, dt) for dt in (np.float32, np.float64))
    got = got.cpu().numpy()
    deg = np.bincount(c["recv"], minlength=c["N"])
    assert np.all(np.isfinite(got)), what
    assert not got[deg == 0].any(), "%s: a receiver without edges is not 0" % what
    print("[cfconv table] %-40s worst row %.2e from float32, %.2e from float64 (restatement %.2e)" % (
        what, rowwise_rel(got, r32), rowwise_rel(got, r64), rowwise_rel(r32, r64)))
    return assert_rows_close(got, r32, r64, what=what)


# degrees whose segments begin and end on tile and half-tile edges (edges 15|16, 31|32, 47|48, 63|64), a receiver over
# three tiles (70 edges from edge 106 on), receivers without edges between them
DEGREES = [16, 16, 0, 32, 15, 1, 1, 15, 0, 0, 10, 70, 3, 0, 29, 32, 16, 1]


@pytest.fixture(scope="module")
def segments():
    return _case(24, T.degree_edges(24, DEGREES, 5, first=2), seed=1)


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("bins,offset", [(20, 0.0), (25, 0.5), (16, 0.0)])
def test_table_rows_and_self_check(bins, offset):
    """Rows within one float32 rounding of the row scale of the float64 filter at the knots (2^-24 of the row's largest
    entry, and 1e-12 for the device's double-precision exp and log1p); padding rows zero; the self-check words give the
    figure the NumPy restatement gives on the same points, to two digits."""
    c = _case(5, T.tile_exact(8, 5)[1], bins=bins, offset=offset)
    lay, table, err = _table(c)
    L = M.layout(bins, c["distance"], c["sigma"], offset)
    assert (lay.n_int, lay.rows, lay.inv_h) == (L["n_int"], L["rows"], 32.0)
    assert lay.v_lo == float(L["v_lo"]) and lay.v_end == float(L["v_end"])
    rows = table.cpu().numpy()
    ref = M.filter64(M.knots(L), c["w1"], c["b1"], c["w2"], c["b2"], c["distance"], c["sigma"])
    scale = np.max(np.abs(ref), axis=1, keepdims=True)
    worst = float(np.max(np.abs(rows[:L["n_int"] + 5] - ref) / scale))
    print("[cfconv table] B=%d offset %.1f: rows off by %.2e of the row scale (2^-24 = %.2e); self-check %.2e" % (
        bins, offset, worst, 2.0 ** -24, err))
    assert worst <= 2.0 ** -24 + 1e-12
    assert not rows[L["n_int"] + 5:].any()
    model = M.error_over_scale(rows, M.check_points(L, offset), offset, L, c["w1"], c["b1"], c["w2"], c["b2"],
                               c["distance"], c["sigma"])
    assert abs(err - model) <= 0.05 * model and err <= FILTER_TABLE_BAR


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("m", [1, 31, 32, 33, 64, 65, 97])
def test_edge_counts(m):
    n, e = T.tile_exact(m, n=5, seed=2)
    c = _case(n, e, seed=m)
    _compare(c, _run(c), "M = %d" % m)


@pytest.mark.parametrize("waves", [0, 4, 8, 16])
def test_segment_layouts(segments, waves):
    """In-degree 70 over three tiles, segments on tile and half-tile edges, receivers without edges - every workgroup size
    (at 16 waves the sender rows go through the eight-row window)."""
    _compare(segments, _run(segments, waves=waves), "segments, waves %d" % waves)


def test_half_grid(segments):
    _compare(segments, _run(segments, flags=16, waves=4), "segments, half grid")


def test_unsorted_list_through_perm():
    c = _case(24, T.degree_edges(24, DEGREES, 6, first=2), seed=2, shuffled=True)
    assert C.kernel_order(c)[1] is not None
    _compare(c, _run(c), "shuffled list")


def test_deterministic_mode(segments):
    tab = _table(segments)
    first = _run(segments, flags=32, tab=tab)
    assert torch.equal(first, _run(segments, flags=32, tab=tab)), "two deterministic runs differ"
    assert torch.equal(first, _run(segments, flags=32, waves=16, tab=tab)), "deterministic runs at 4 and 16 waves differ"
    _compare(segments, first, "segments, deterministic")


@pytest.mark.parametrize("offset", [0.0, 0.5])
def test_distances_at_the_ends_of_the_domain(offset):
    """d = 0, 1e-6, on a knot, mid-interval, at v_hi, just beyond it, 10 and 1e3 (every special value on four edges)."""
    n, e = T.tile_exact(97, n=7, seed=3)
    c = _case(n, e, offset=offset, seed=3)
    L = M.layout(c["bins"], c["distance"], c["sigma"], offset)
    end = f32(L["v_end"] + f32(offset))
    special = np.array([0.0, 1e-6, offset + float(L["v_lo"]) + 17 * L["h"], offset + float(L["v_lo"]) + 17.5 * L["h"], end,
                        np.nextafter(end, f32(np.inf)), 10.0, 1e3], f32)
    c["dist"] = c["dist"].copy()
    c["dist"][:4 * len(special)] = np.tile(special, 4)
    _compare(c, _run(c), "special distances, offset %.1f" % offset)


@pytest.mark.parametrize("bins", [20, 25, 16])
def test_basis_sizes(bins):
    """20 and 25 (the MFMA kernel's fixed builds) and 16 (its generic FP32 build): one table kernel serves them all."""
    n, e = T.tile_exact(65, n=6, seed=bins)
    c = _case(n, e, bins=bins, seed=4)
    _compare(c, _run(c), "B = %d" % bins)


def test_offset(segments):
    c = dict(segments, offset=0.5)
    _compare(c, _run(c), "segments, offset 0.5")


def test_table_kernel_against_mfma_kernel(segments):
    """Same inputs, both kernels: every row within the bar times the row scale (module docstring)."""
    c = segments
    got = _run(c).cpu().numpy().astype(np.float64)
    packed = torch.empty(_ffi.lib().mp_cfconv_packed_floats(), dtype=torch.float32, device="cuda")
    w = [_dev(c[k]) for k in ("w1", "b1", "w2", "b2")]
    _ffi.call("mp_cfconv_pack_f32", _ffi.ptr(w[0]), _ffi.ptr(w[1]), c["bins"], _ffi.ptr(w[2]), _ffi.ptr(w[3]),
              _ffi.ptr(packed), _ffi.stream())
    t = {k: _dev(c[k]) for k in ("x", "dist", "recv", "send")}
    out = torch.zeros((c["N"], F), dtype=torch.float32, device="cuda")
    _ffi.call("mp_cfconv_gauss_fused_f32", _ffi.ptr(t["x"]), c["N"], _ffi.ptr(t["dist"]), c["bins"], c["distance"],
              c["sigma"], c["offset"], _ffi.ptr(packed), _ffi.ptr(t["recv"]), _ffi.ptr(t["send"]), None, c["M"], 1,
              _ffi.ptr(out), _ffi.stream())
    torch.cuda.synchronize()
    mfma = out.cpu().numpy().astype(np.float64)
    filt = M.filter64(c["dist"] - f32(c["offset"]), c["w1"], c["b1"], c["w2"], c["b2"], c["distance"], c["sigma"])
    row_scale = np.zeros(c["N"])
    np.add.at(row_scale, c["recv"], np.max(np.abs(c["x"][c["send"]]), axis=1) * np.max(np.abs(filt)))
    has = row_scale > 0
    worst = float(np.max(np.max(np.abs(got - mfma), axis=1)[has] / row_scale[has]))
    print("[cfconv table] table kernel against MFMA kernel: worst row %.2e of the row scale (bar %.2e)" % (
        worst, FILTER_TABLE_BAR))
    assert worst <= FILTER_TABLE_BAR
    assert not got[~has].any() and not mfma[~has].any()


# ------------------------------------------------------------------------------------------------ the route
def _model(p):
    from gcnn_keras_amd.literature import Schnet
    model = Schnet.make_model(depth=3)
    model.set_weights(list(p.values()))
    return model


def _oracle(p, b):
    return ko.schnet_forward(p, ko.R(b["node_number"], b["node_splits"]), ko.R(b["node_coordinates"], b["node_splits"]),
                             ko.R(b["edge_indices"], b["edge_splits"]), depth=3)


@pytest.fixture(scope="module")
def params():
    return synth.schnet_params(seed=7, random_bias=True)


def test_route_lone_forward_group_members_and_replay(params):
    """The table route is on by default; a lone forward and the members of a three-batch launch group agree as the
    existing group tests ask (2e-6 per row: the cfconv boundary sums pair differently), the direct launch of first sight
    and the replayed graph give equal bits, everything against the oracle."""
    model = _model(params)
    batches = [synth.qm9_like_batch(num_graphs=g, seed=s) for g, s in ((6, 11), (9, 12), (4, 13))]
    ins = [mol_inputs(b) for b in batches]
    first = [model(x) for x in ins]
    assert model.fused.last == "direct" and model.fused.filter_table_active
    replay = [model(x) for x in ins]
    assert model.fused.last == "graph"
    group = model.fused.call_group(ins)
    group_replay = model.fused.call_group(ins)
    torch.cuda.synchronize()
    slot = model.fused.slot_of(ins[0])
    assert slot.filter_table_active and "cfconv_table_kernel" in slot.roofline(8000.0, 157.3, iters=2)["kernel"]
    for k, b in enumerate(batches):
        assert torch.equal(first[k], replay[k]), "member %d: direct launch and replay differ" % k
        assert torch.equal(group[k], group_replay[k])
        assert rowwise_rel(group[k].cpu().numpy(), first[k].cpu().numpy()) <= 2e-6
        assert_rows_close(first[k].cpu().numpy(), _oracle(params, b), what="table route, batch %d" % k)
    model.fused.check_flags()


_CHILD = """
import json, sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from gcnn_keras_amd import synth
from gcnn_keras_amd.literature import Schnet
from helpers import mol_inputs
p = synth.schnet_params(seed=7, random_bias=True)
model = Schnet.make_model(depth=3)
model.set_weights(list(p.values()))
out = model(mol_inputs(synth.qm9_like_batch(num_graphs=9, seed=12)))
print(json.dumps({"active": bool(model.fused.filter_table_active), "out": out.cpu().numpy().reshape(-1).tolist()}))
"""


def test_route_switched_off_in_a_child_process(params):
    """``MPENGINE_FILTER_TABLE=0`` keeps the MFMA kernel: predictions within 1e-5 per row of the table route's."""
    model = _model(params)
    b = synth.qm9_like_batch(num_graphs=9, seed=12)
    table = model(mol_inputs(b)).cpu().numpy()
    assert model.fused.filter_table_active
    env = dict(os.environ, MPENGINE_FILTER_TABLE="0")
    res = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, check=True,
                         capture_output=True, text=True)
    got = json.loads(res.stdout.strip().splitlines()[-1])
    assert got["active"] is False
    mfma = np.asarray(got["out"], np.float32).reshape(-1, 1)
    err = rowwise_rel(table, mfma)
    print("[cfconv table] table route against MPENGINE_FILTER_TABLE=0: worst row %.2e" % err)
    assert err <= 1e-5


def test_weight_update_flips_the_route_and_back(params):
    """``set_weights`` with ``W1`` x 20 in one block: that block's table misses its self-check, the whole route runs the
    MFMA kernel (captured graphs dropped), the forward matches the oracle; the old weights bring the table back."""
    model = _model(params)
    b = synth.qm9_like_batch(num_graphs=7, seed=14)
    x = mol_inputs(b)
    before = [model(x) for _ in range(2)][-1]                  # the second call replays the captured graph
    assert model.fused.filter_table_active and model.fused.last == "graph"
    extreme = dict(params)
    extreme["interaction1/cfconv/dense1/kernel"] = params["interaction1/cfconv/dense1/kernel"] * f32(20.0)
    model.set_weights(list(extreme.values()))
    outs = [model(x) for _ in range(2)]
    assert not model.fused.filter_table_active
    slot = model.fused.slot_of(x)
    assert "cfconv_fused_kernel" in slot.roofline(8000.0, 157.3, iters=2)["kernel"]
    errs = model.fused._packed["ftable"]["err"]
    assert errs[1] > FILTER_TABLE_BAR and errs[0] <= FILTER_TABLE_BAR and errs[2] <= FILTER_TABLE_BAR
    for out in outs:
        assert_rows_close(out.cpu().numpy(), _oracle(extreme, b), what="fall-back after the weight update")
    model.set_weights(list(params.values()))
    after = [model(x) for _ in range(2)]
    assert model.fused.filter_table_active
    for out in after:
        assert torch.equal(out, before)
    model.fused.check_flags()
