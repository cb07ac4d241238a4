"""The PaiNN kernels of csrc/mp_painn_fused.hip (stage 0, the two LDS-tile message kernels, the gather pair, the geometry
reverse kernel) and the fused update pair of csrc/mp_chain.hip off the molecular shapes, kernel by kernel through the C ABI
with the argument lists of ``FusedPainn._forward`` / ``_backward``, against the float64 restatements of
tests/painn_cases.py, and three composed runs.  Every output buffer is filled with NaN and carries a tail behind its
logical end that must still be NaN afterwards; tile tables always come from ``message_tile_table``.

Bars (none of its own): the defaults of ``parity.assert_rows_close`` with the float64 twin for every node-row output and
the stage 0 rows; 2e-5 of the tensor's largest magnitude for the per-edge scalars ``g_d`` / ``g_rij`` (``_close`` of
tests/test_gpu_schnet_bwd.py); 1e-5 of the largest force for mp_edge_geometry_bwd_f32 (the force test there);
``assert_rows_close`` / ``assert_forces_close`` with defaults for the composed runs.

Case -> branch.  ``steps`` (consecutive degrees 0 1 7 8 9 15 16 17 31 32 33 47 0 33 16 17 and reversed, 1 2 3 5 16 receivers
or 1 2 3 senders per tile): pairs whose members take a different number of 16-edge steps, the 8-edge half step, an odd
tile.  ``odd-47`` (graphs of 0 1 2 3 0 5 47 0 nodes, up to 47 receivers per tile) and ``odd`` (... 63 nodes; reverse tiles
and gather): a last pair of one receiver, empty graphs.  ``slots`` (sender degrees 1 4 5 8 9 12 13 16 17 33, up to 16
senders per tile, one self loop): every ``painn_bwd_slots<G>`` path and a second step into the same slab.  ``rounds``
(degrees 63 64 65 130): the ``EC`` tails and further 64-edge rounds of the gather pair, also at 32 basis functions
without ``bw``.  ``complete49 / 50 / 48-b31 / 56 / 57``: the last graphs that fit LDS and the first that do not.
``trip-tiles`` (2100 graphs): a second trip of the tile loops.  ``trip-waves`` (8209 nodes): a second trip of the wave
loops.  ``steps-b1 / b7 / b8``: one k group, the group boundary.  The 62-node clamp of a tile is out of reach: the rows
of a graph bound a forward tile to 49 receivers at 20 basis functions, a reverse tile to about 30 senders.

Distance of the float32 restatement from its float64 twin on these cases, in the metric of the comparison (torch / NumPy,
CPU; asserted at or below half the bar by tests/test_painn_cases.py, which prints each figure):

  stage 0, 1023 / 1030 graphs of 1..3 atoms        dist 1.2e-07, rij 1.4e-07, rbf 2.7e-06, rbfd 4.0e-06, env 2.5e-07,
                                                   envd 1.7e-07, z0 and v0 exact
  message forward ds / dv rows                     steps (all variants) <= 4.9e-07; odd, odd-47 <= 2.5e-07; rounds <= 5.2e-07;
                                                   complete 48 49 50 <= 4.3e-07; trip-tiles, trip-waves <= 3.9e-07
  message reverse g_s / g_v rows                   <= 4.9e-07 on every case
  message reverse g_d / g_rij                      <= 6.9e-07 / <= 1.8e-07 of the largest magnitude on every case
  geometry reverse, hubs 64 65 100 1000 / ring     <= 3.0e-07 / 9.3e-08 of the largest force
  update z2 v2 h2 c prod a, N = 1 15 16 17 4097    <= 1.6e-06; reverse g_zp g_uv <= 1.9e-06 (with and without g_v2, biases)
  models: 49 + 21, 52 + 21 atoms, 2100 molecules   energies 2.1e-06, 6.8e-07, 3.0e-06; forces 1.3e-06, 1.4e-06, 3.9e-06 of a
                                                   molecule's scale, worst atom row 9.3e-06, 7.9e-06, 6.9e-06 (half bar 1e-05)
"""
import functools

import numpy as np
import pytest
import torch

import painn_cases as C
from gcnn_keras_amd import _ffi, synth
from gcnn_keras_amd.fused_painn import message_tile_table
from helpers import mol_inputs, painn_weight_list
from oracle import kgcnn_oracle as ko
from oracle import torch_force_oracle as tfo
from parity import assert_forces_close, assert_rows_close

pytestmark = pytest.mark.gpu

TAIL = 5      # elements / rows behind the logical end of every output buffer
F = C.F


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan(rows, *inner):
    return torch.full((rows + TAIL,) + inner, float("nan"), dtype=torch.float32, device="cuda")


def _tail_is_nan(buf, rows, what):
    assert bool(torch.isnan(buf[rows:]).all()), "%s: a store past row %d" % (what, rows)


def _rows(buf, rows, ref32, ref64, what):
    """Node-row output: exactly ``rows`` rows written and finite, ``assert_rows_close`` with its defaults."""
    _tail_is_nan(buf, rows, what)
    got = buf[:rows].cpu().numpy().reshape(np.shape(ref64))
    assert np.all(np.isfinite(got)), "%s: %d elements unwritten or not finite" % (what, int(np.sum(~np.isfinite(got))))
    err = assert_rows_close(got, ref32, ref64, what=what)
    print("[edges] %s: rows %.2e from the float32 restatement" % (what, err))


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


def _filter_image(c, t):
    image = torch.empty(_ffi.MP_PAINN_FILTER_IMAGE_BYTES, dtype=torch.uint8, device="cuda")
    _ffi.call("mp_painn_filter_pack_f32", _ffi.ptr(t["Ww"]), _ffi.ptr(t["bw"]), c["B"], _ffi.ptr(image), _ffi.stream())
    torch.cuda.synchronize()
    return image


def _tiles(c, column, per, reverse):
    ptr, _ = C.csr(c[column], c["N"])
    tl = message_tile_table(c["node_splits"], ptr, c["B"], per=per, reverse=reverse)
    assert tl is not None, (c["name"], per)
    tl["table"] = _dev(tl["table"])
    return tl


# ------------------------------------------------------------------------------------- A. message, forward
@functools.lru_cache(maxsize=None)
def _forward_refs(name):
    c = C.message_case(**C.FORWARD_RUNS[name][0])
    return c, C.message_forward_restate(c, np.float32), C.message_forward_restate(c, np.float64)


def _forward_operands(c):
    t = {k: _dev(c[k]) for k in ("s", "v", "rbf", "env", "rij", "Ww", "bw", "send", "z_in")}
    ptr0, perm0 = C.csr(c["recv"], c["N"])
    t["ptr0"], t["perm0"] = _dev(ptr0), _dev(perm0)
    return t


def _forward(c, t, tl=None, image=None):
    n, m = c["N"], c["M"]
    ds, dv = _nan(n, F), _nan(n, 3, F)
    if tl is not None:
        _ffi.call("mp_painn_message_tiles_f32", _ffi.ptr(t["s"]), _ffi.ptr(t["v"]), n, _ffi.ptr(t["rbf"]), c["B"],
                  _ffi.ptr(t["env"]), _ffi.ptr(t["rij"]), _ffi.ptr(image), _ffi.ptr(t["ptr0"]), _ffi.ptr(t["send"]), m,
                  _ffi.ptr(tl["table"]), tl["count"], tl["max_rows"], tl["max_edges"], _ffi.ptr(t["z_in"]), _ffi.ptr(ds),
                  _ffi.ptr(dv), _ffi.stream())
    else:
        _ffi.call("mp_painn_message_f32", _ffi.ptr(t["s"]), _ffi.ptr(t["v"]), n, _ffi.ptr(t["rbf"]), c["B"], _ffi.ptr(t["env"]),
                  _ffi.ptr(t["rij"]), _ffi.ptr(t["Ww"]), _ffi.ptr(t["bw"]), _ffi.ptr(t["ptr0"]), _ffi.ptr(t["perm0"]),
                  _ffi.ptr(t["send"]), m, _ffi.ptr(t["z_in"]), _ffi.ptr(ds), _ffi.ptr(dv), _ffi.stream())
    torch.cuda.synchronize()
    return ds, dv


@pytest.mark.parametrize("name", sorted(C.FORWARD_RUNS))
def test_message_forward(name):
    """``ds`` / ``dv`` of the gather kernel on every case and of the tile kernel at every listed tile size, against the
    float64 restatement and against each other; each called twice (fixed summation order: the same bits)."""
    c, (ds32, dv32), (ds64, dv64) = _forward_refs(name)
    pers = C.FORWARD_RUNS[name][1]
    n, t = c["N"], _forward_operands(c)
    assert (t["perm0"] is None) or not pers                         # the tile kernel takes receiver-sorted lists only
    gather = _forward(c, t)
    again = _forward(c, t)
    assert torch.equal(gather[0][:n], again[0][:n]) and torch.equal(gather[1][:n], again[1][:n])
    _rows(gather[0], n, ds32, ds64, "forward gather %s ds" % name)
    _rows(gather[1], n, dv32, dv64, "forward gather %s dv" % name)
    silent = np.diff(C.csr(c["recv"], n)[0]) == 0
    if c["z_in"] is None:                                           # a node without edges: exact zeros
        assert not bool(gather[0][:n][_dev(silent)].any()) and not bool(gather[1][:n][_dev(silent)].any())
    image = _filter_image(c, t) if pers else None
    for per in pers:
        tl = _tiles(c, "recv", per, False)
        tag = "forward tiles %s per=%s (%d tiles of <= %d)" % (name, per, tl["count"], tl["max_own"])
        ds, dv = _forward(c, t, tl, image)
        ds2, dv2 = _forward(c, t, tl, image)
        _rows(ds, n, ds32, ds64, tag + " ds")
        _rows(dv, n, dv32, dv64, tag + " dv")
        assert torch.equal(ds[:n], ds2[:n]) and torch.equal(dv[:n], dv2[:n]), tag + ": two calls differ"
        assert_rows_close(ds[:n].cpu().numpy(), gather[0][:n].cpu().numpy(), ds64, what=tag + " ds against gather")
        assert_rows_close(dv[:n].cpu().numpy(), gather[1][:n].cpu().numpy(), dv64, what=tag + " dv against gather")
        if c["z_in"] is None:
            assert not bool(ds[:n][_dev(silent)].any()) and not bool(dv[:n][_dev(silent)].any())


# ------------------------------------------------------------------------------------- B. message, reverse
@functools.lru_cache(maxsize=None)
def _reverse_refs(name):
    c = C.message_case(**C.REVERSE_RUNS[name][0])
    return c, C.message_reverse_restate(c, np.float32), C.message_reverse_restate(c, np.float64)


def _reverse_operands(c):
    t = {k: _dev(c[k]) for k in ("s", "v", "rbf", "rbfd", "env", "envd", "rij", "Ww", "bw", "recv", "g_ds", "g_dv")}
    ptr1, perm1 = C.csr(c["send"], c["N"])
    t["ptr1"], t["perm1"] = _dev(ptr1), _dev(perm1)
    return t


def _reverse_buffers(c, slices):
    n, m = c["N"], c["M"]
    return {"g_s": _nan(n, 3 * F), "g_v": _nan(n, 3, F), "g_d": _nan(slices * m), "g_rij": _nan(slices * m, 3)}


def _reverse(c, t, out, tl=None, image=None, accumulate=0, with_g_v=True):
    n, m = c["N"], c["M"]
    g_v = _ffi.ptr(out["g_v"]) if with_g_v else None
    if tl is not None:
        _ffi.call("mp_painn_message_bwd_tiles_f32", _ffi.ptr(t["s"]), _ffi.ptr(t["v"]), n, _ffi.ptr(t["rbf"]), _ffi.ptr(t["rbfd"]),
                  c["B"], _ffi.ptr(t["env"]), _ffi.ptr(t["envd"]), _ffi.ptr(t["rij"]), _ffi.ptr(image), _ffi.ptr(t["ptr1"]),
                  _ffi.ptr(t["perm1"]), _ffi.ptr(t["recv"]), m, _ffi.ptr(tl["table"]), tl["count"], tl["max_rows"],
                  tl["max_own"], tl["max_edges"], _ffi.ptr(t["g_ds"]), _ffi.ptr(t["g_dv"]), _ffi.ptr(out["g_s"]), g_v,
                  _ffi.ptr(out["g_d"]), _ffi.ptr(out["g_rij"]), accumulate, _ffi.stream())
    else:
        _ffi.call("mp_painn_message_bwd_f32", _ffi.ptr(t["s"]), _ffi.ptr(t["v"]), n, _ffi.ptr(t["rbf"]), _ffi.ptr(t["rbfd"]),
                  c["B"], _ffi.ptr(t["env"]), _ffi.ptr(t["envd"]), _ffi.ptr(t["rij"]), _ffi.ptr(t["Ww"]), _ffi.ptr(t["bw"]),
                  _ffi.ptr(t["ptr1"]), _ffi.ptr(t["perm1"]), _ffi.ptr(t["recv"]), m, _ffi.ptr(t["g_ds"]), _ffi.ptr(t["g_dv"]),
                  _ffi.ptr(out["g_s"]), g_v, _ffi.ptr(out["g_d"]), _ffi.ptr(out["g_rij"]), accumulate, _ffi.stream())
    torch.cuda.synchronize()
    return out


def _check_reverse(c, out, slices, r32, r64, tag):
    n, m = c["N"], c["M"]
    _rows(out["g_s"], n, r32["g_s"], r64["g_s"], tag + " g_s")
    _rows(out["g_v"], n, r32["g_v"], r64["g_v"], tag + " g_v")
    _tail_is_nan(out["g_d"], slices * m, tag + " g_d")
    _tail_is_nan(out["g_rij"], slices * m, tag + " g_rij")
    g_d = out["g_d"][:slices * m].reshape(slices, m)
    g_rij = out["g_rij"][:slices * m].reshape(slices, m, 3)
    assert bool(torch.isfinite(g_d).all()) and bool(torch.isfinite(g_rij).all()), tag + ": a slice entry unwritten"
    _close(g_d.double().sum(0), r64["g_d"], C.BAR_EDGE, tag + " g_d")
    _close(g_rij.double().sum(0), r64["g_rij"], C.BAR_EDGE, tag + " g_rij")


def _same_bits(a, b, c, slices):
    n, m = c["N"], slices * c["M"]
    return all(torch.equal(a[k][:rows], b[k][:rows]) for k, rows in (("g_s", n), ("g_v", n), ("g_d", m), ("g_rij", m)))


@pytest.mark.parametrize("name", sorted(C.REVERSE_RUNS))
def test_message_reverse(name):
    """``g_s``, ``g_v``, ``g_d``, ``g_rij`` of the gather kernel (two slices, added here) on every case and of the tile
    kernel (one slice) at every listed tile size, sender-sorted lists and lists that need ``perm1``, against the float64
    restatement; each called twice (the same bits)."""
    c, r32, r64 = _reverse_refs(name)
    pers = C.REVERSE_RUNS[name][1]
    t = _reverse_operands(c)
    assert (t["perm1"] is not None) == ("shuffled" in name)
    gather = _reverse(c, t, _reverse_buffers(c, 2))
    assert _same_bits(gather, _reverse(c, t, _reverse_buffers(c, 2)), c, 2), name + ": two gather calls differ"
    _check_reverse(c, gather, 2, r32, r64, "reverse gather %s" % name)
    image = _filter_image(c, t) if pers else None
    for per in pers:
        tl = _tiles(c, "send", per, True)
        tag = "reverse tiles %s per=%s (%d tiles of <= %d)" % (name, per, tl["count"], tl["max_own"])
        out = _reverse(c, t, _reverse_buffers(c, 1), tl, image)
        again = _reverse(c, t, _reverse_buffers(c, 1), tl, image)
        _check_reverse(c, out, 1, r32, r64, tag)
        assert _same_bits(out, again, c, 1), tag + ": two calls differ"


@pytest.mark.parametrize("kernel", ["tiles", "gather"])
def test_message_reverse_accumulate_and_null_g_v(kernel):
    """``accumulate = 1`` adds exactly the bits the first call wrote to ``g_d`` / ``g_rij`` (``g_s`` and ``g_v`` are written
    again, not added to); a null ``g_v`` leaves a NaN-filled buffer untouched and changes nothing else."""
    c, r32, r64 = _reverse_refs("slots")
    t = _reverse_operands(c)
    slices = 1 if kernel == "tiles" else 2
    tl = _tiles(c, "send", 3, True) if kernel == "tiles" else None
    image = _filter_image(c, t) if kernel == "tiles" else None
    m = slices * c["M"]
    out = _reverse(c, t, _reverse_buffers(c, slices), tl, image, accumulate=0)
    first = {k: v.clone() for k, v in out.items()}
    _check_reverse(c, first, slices, r32, r64, "reverse %s slots, written" % kernel)
    _reverse(c, t, out, tl, image, accumulate=1)
    assert torch.equal(out["g_d"][:m], first["g_d"][:m] + first["g_d"][:m])
    assert torch.equal(out["g_rij"][:m], first["g_rij"][:m] + first["g_rij"][:m])
    assert torch.equal(out["g_s"][:c["N"]], first["g_s"][:c["N"]]) and torch.equal(out["g_v"][:c["N"]], first["g_v"][:c["N"]])
    for k, rows in (("g_s", c["N"]), ("g_v", c["N"]), ("g_d", m), ("g_rij", m)):
        _tail_is_nan(out[k], rows, "accumulate " + k)
    bare = _reverse(c, t, _reverse_buffers(c, slices), tl, image, with_g_v=False)
    assert bool(torch.isnan(bare["g_v"]).all())
    assert all(torch.equal(bare[k][:rows], first[k][:rows]) for k, rows in (("g_s", c["N"]), ("g_d", m), ("g_rij", m)))


# ------------------------------------------------------------------------------------- C. geometry reverse
@pytest.mark.parametrize("name", sorted(C.geometry_cases()))
def test_geometry_reverse(name):
    """mp_edge_geometry_bwd_f32 alone (``g_d`` / ``g_rij`` are given random slices): hubs of 64, 65, 100 and 1000 edges on
    either column with and without permutations, one and two slices, self loops and a coincident pair (d = 0), 8209 nodes
    most of which are isolated (second node trip)."""
    c = C.geometry_case(**C.geometry_cases()[name])
    n, m, e = c["N"], c["M"], c["edges"]
    (ptr0, perm0), (ptr1, perm1) = C.csr(e[:, 0], n), C.csr(e[:, 1], n)
    t = {k: _dev(c[k]) for k in ("g_d", "g_rij", "rij", "dist")}
    t.update(ptr0=_dev(ptr0), perm0=_dev(perm0), ptr1=_dev(ptr1), perm1=_dev(perm1))
    assert (perm0 is None) == bool(np.all(np.diff(e[:, 0]) >= 0)) and (perm1 is None) == bool(np.all(np.diff(e[:, 1]) >= 0))
    out = _nan(n, 3)
    for _ in range(2):
        _ffi.call("mp_edge_geometry_bwd_f32", _ffi.ptr(t["g_d"]), _ffi.ptr(t["g_rij"]), c["slices"], _ffi.ptr(t["rij"]),
                  _ffi.ptr(t["dist"]), _ffi.ptr(t["ptr0"]), _ffi.ptr(t["perm0"]), _ffi.ptr(t["ptr1"]), _ffi.ptr(t["perm1"]),
                  n, m, c["scale"], _ffi.ptr(out), _ffi.stream())
        torch.cuda.synchronize()
    _tail_is_nan(out, n, name)
    got = out[:n].cpu().numpy()
    touched = np.zeros(n, bool)
    touched[e.reshape(-1)] = True
    assert np.all(np.isfinite(got)) and np.all(got[~touched] == 0)             # isolated nodes: exact zeros
    _close(out[:n], C.geometry_restate(c, np.float64), C.BAR_FORCE, "geometry reverse " + name)


# ------------------------------------------------------------------------------------- D. stage 0
@pytest.mark.parametrize("name", sorted(C.STAGE0_RUNS))
def test_stage0(name):
    """mp_painn_stage0_f32 on 1023 graphs (row_splits searched in LDS) and 1030 (the ``<false>`` build), float32 and int64
    node numbers (two outside the embedding table), with and without the cosine envelope, three edges beyond the Bessel
    cutoff; out-of-range edge ids are clamped into their graph and raise the flag."""
    c = C.stage0_case(**C.STAGE0_RUNS[name])
    r32, r64 = C.stage0_restate(c, np.float32), C.stage0_restate(c, np.float64)
    n, m, b = c["N"], c["M"], c["B"]
    t = {k: _dev(c[k]) for k in ("numbers", "emb", "idx", "node_splits", "edge_splits", "xyz", "freq")}
    ids = {k: torch.full((m + TAIL,), -7, dtype=torch.int32, device="cuda") for k in ("recv", "send")}
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = {"z0": _nan(n, F), "v0": _nan(n, 3, F), "dist": _nan(m), "rij": _nan(m, 3), "rbf": _nan(m, b), "rbfd": _nan(m, b),
           "env": _nan(m), "envd": _nan(m)}
    _ffi.call("mp_painn_stage0_f32", _ffi.ptr(t["numbers"]), 1 if c["numbers"].dtype == np.int64 else 0, n, _ffi.ptr(t["emb"]),
              c["vocab"], c["v_init"], _ffi.ptr(out["z0"]), _ffi.ptr(out["v0"]), _ffi.ptr(t["idx"]), m,
              _ffi.ptr(t["node_splits"]), _ffi.ptr(t["edge_splits"]), c["G"], _ffi.ptr(t["xyz"]), _ffi.ptr(t["freq"]), b,
              c["cutoff"], c["exponent"], c["cos_cutoff"], _ffi.ptr(ids["recv"]), _ffi.ptr(ids["send"]), _ffi.ptr(flags),
              _ffi.ptr(out["dist"]), _ffi.ptr(out["rij"]), _ffi.ptr(out["rbf"]), _ffi.ptr(out["rbfd"]), _ffi.ptr(out["env"]),
              _ffi.ptr(out["envd"]), _ffi.stream())
    torch.cuda.synchronize()
    assert bool(int(flags.item()) & _ffi.MP_FLAG_OOB) == bool(len(c["marked"])), name
    for k in ("recv", "send"):
        assert np.array_equal(ids[k][:m].cpu().numpy(), r64[k]) and bool((ids[k][m:] == -7).all()), k
    for k, rows in (("z0", n), ("v0", n), ("dist", m), ("rij", m), ("rbf", m), ("rbfd", m), ("env", m), ("envd", m)):
        if r64[k] is None:                                          # no envelope asked for: the buffers stay untouched
            assert bool(torch.isnan(out[k]).all()), k
        else:
            _rows(out[k], rows, r32[k], r64[k], "stage 0 %s %s" % (name, k))
    far = r64["dist"] >= c["cutoff"]
    assert far.sum() == 6 and not bool(out["rbf"][:m][_dev(far)].any()) and not bool(out["rbfd"][:m][_dev(far)].any())
    assert np.array_equal(out["z0"][:n].cpu().numpy(), r32["z0"]) and np.array_equal(out["v0"][:n].cpu().numpy(), r32["v0"])


# ------------------------------------------------------------------------------------- E. update pair
def _chain_image(w):
    w = _dev(w)
    out = torch.empty(w.numel(), dtype=torch.float32, device="cuda")
    _ffi.call("mp_chain_pack_f32", _ffi.ptr(w), int(w.shape[0]), int(w.shape[1]), _ffi.ptr(out), _ffi.stream())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("n,bias", C.UPDATE_RUNS)
def test_update_pair(n, bias):
    """mp_painn_update_fused_f32 with every saved output given (forces) and all of them null (energy only), and
    mp_painn_update_fused_bwd_f32 with and without ``g_v2``: node counts around the 16-row tile and one past the 256
    persistent tiles, biases present and absent."""
    c = C.update_case(n, bias=bias)
    f32, f64 = C.update_forward_restate(c, np.float32), C.update_forward_restate(c, np.float64)
    tag = "update N=%d%s" % (n, "" if bias else " no bias")
    t = {k: _dev(c[k]) for k in ("zp", "vp", "uv", "bd", "ba", "g_z2", "g_v2")}
    img = {"Wd": _chain_image(c["Wd"]), "Wa": _chain_image(c["Wa"]), "WaT": _chain_image(c["Wa"].T),
           "WdT": _chain_image(c["Wd"].T)}
    widths = {"z2": (F,), "v2": (3, F), "h2": (F,), "c": (2 * F,), "prod": (F,), "a": (3 * F,)}
    results = {}
    for saved in (True, False):
        out = {k: _nan(n, *w) for k, w in widths.items()}
        opt = lambda k: _ffi.ptr(out[k]) if saved else None
        _ffi.call("mp_painn_update_fused_f32", _ffi.ptr(t["zp"]), _ffi.ptr(t["vp"]), _ffi.ptr(t["uv"]), n, _ffi.ptr(img["Wd"]),
                  _ffi.ptr(t["bd"]), C.ACT_SWISH, 0.0, opt("h2"), _ffi.ptr(img["Wa"]), _ffi.ptr(t["ba"]), opt("c"), opt("prod"),
                  opt("a"), _ffi.ptr(out["z2"]), _ffi.ptr(out["v2"]), _ffi.stream())
        torch.cuda.synchronize()
        for k in C.UPDATE_OUTPUTS:
            if saved or k in ("z2", "v2"):
                _rows(out[k], n, f32[k], f64[k], "%s %s%s" % (tag, k, "" if saved else " (nothing saved)"))
            else:
                assert bool(torch.isnan(out[k]).all()), k
        results[saved] = out
    assert all(torch.equal(results[True][k][:n], results[False][k][:n]) for k in ("z2", "v2"))
    assert np.array_equal(results[True]["c"][:n, :F].cpu().numpy(), c["zp"])                    # c = [z | norm]
    saved = {k: _dev(f64[k].astype(np.float32)) for k in ("prod", "a", "c", "h2")}
    for with_g_v2 in (True, False):
        r32, r64 = (C.update_reverse_restate(c, dt, with_g_v2) for dt in (np.float32, np.float64))
        g_zp, g_uv = _nan(n, F), _nan(3 * n, 2 * F)
        _ffi.call("mp_painn_update_fused_bwd_f32", _ffi.ptr(t["g_z2"]), _ffi.ptr(t["g_v2"]) if with_g_v2 else None,
                  _ffi.ptr(t["uv"]), _ffi.ptr(saved["prod"]), _ffi.ptr(saved["a"]), _ffi.ptr(saved["c"]), n, _ffi.ptr(img["WaT"]),
                  C.ACT_SWISH, 0.0, _ffi.ptr(saved["h2"]), _ffi.ptr(img["WdT"]), _ffi.ptr(g_zp), _ffi.ptr(g_uv), _ffi.stream())
        torch.cuda.synchronize()
        end = "" if with_g_v2 else " without g_v2"
        _rows(g_zp, n, r32["g_zp"], r64["g_zp"], "%s reverse%s g_zp" % (tag, end))
        _rows(g_uv, 3 * n, r32["g_uv"], r64["g_uv"], "%s reverse%s g_uv" % (tag, end))


# ------------------------------------------------------------------------------------- F. composed
@pytest.mark.parametrize("name", sorted(C.MODEL_BATCHES))
def test_painn_energy_force_across_the_lds_limit_and_the_tile_grid(name):
    """``PAiNN.make_model`` under ``EnergyForceModel`` on a complete 49-atom molecule next to a 21-atom one (tiles both
    ways), the same with 52 atoms (gather forward, sender tiles in the reverse pass: the slice counts of ``g_d`` / ``g_rij``
    differ between the two kernels) and on 2100 molecules of 2 to 3 atoms (more than 2048 tiles both ways): energies
    against the NumPy oracle, every atom's force against the analytic reference, three calls with the same bits."""
    from gcnn_keras_amd.literature import PAiNN
    from gcnn_keras_amd.model.force import EnergyForceModel
    b = C.model_batch(name, synth.radius_graph)
    p = synth.painn_params(seed=8, random_bias=True)
    energy = PAiNN.make_model(equiv_initialize_kwargs={"dim": 3, "method": "eps"})
    energy.set_weights(painn_weight_list(p))
    assert energy.fused is not None
    model = EnergyForceModel(model_energy=energy, coordinate_input=1, energy_output=0, output_to_tensor=False,
                             output_squeeze_states=True)
    x = mol_inputs(b)
    outs = [model(x) for _ in range(3)]
    assert energy.fused.last == "graph"
    slot = energy.fused.slot_of(x, grad=True)
    assert (slot.tiles0 is not None) == (name != "mixed-route") and slot.tiles1 is not None
    if name == "trip-tiles":
        assert slot.tiles0["count"] > C.TILE_GRID and slot.tiles1["count"] > C.TILE_GRID
    eng, force = outs[0]["energy"].cpu().numpy(), outs[0]["force"].values.cpu().numpy()
    for o in outs[1:]:
        assert torch.equal(o["energy"], outs[0]["energy"]) and torch.equal(o["force"].values, outs[0]["force"].values)
    ns = b["node_splits"]
    assert eng.shape == (len(ns) - 1, 1) and force.shape == (int(ns[-1]), 3)
    e32, e64 = (ko.painn_forward(ko.to_dtype(p, dt), ko.R(b["node_number"], ns), ko.R(b["node_coordinates"].astype(dt), ns),
                                 ko.R(b["edge_indices"], b["edge_splits"]), depth=3, equiv_method="eps", cutoff=None)
                for dt in (np.float32, np.float64))
    assert_rows_close(eng, e32, e64, what="PaiNN %s energy" % name)
    f32, f64 = (tfo.painn_energy_force(p, b, dt, equiv_method="eps", cutoff=None)[1] for dt in (torch.float32, torch.float64))
    assert_forces_close(force, f32, f64, ns, what="PaiNN %s forces" % name)
    energy.fused.check_flags()
