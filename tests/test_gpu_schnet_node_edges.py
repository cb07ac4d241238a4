"""The inference builds of the SchNet node chains (csrc/mp_schnet_node.hip), kernel by kernel through the C ABI, on the
cases of tests/schnet_node_cases.py:

  A  mp_schnet_node_update_f32 (MID) and mp_schnet_node_last_f32 (LAST) with flags 2, 3 (FP32 matrix instructions), 66, 67
     (bf16 pieces, eight waves) and 66|512, 67|512 (half grid) at 1, 15, 16, 17 nodes, one node past the persistent grid
     of each family (8193 / 4097), and around the half-grid switch (4080: 255 tiles, full grid; 4081: 256 tiles, two per
     workgroup, the last of one row; 4097: one workgroup takes three); every bias absent; pre-activations out to +-30.
     The half-grid outputs equal the full-grid ones bit for bit; at flags 2 and 3 the inference builds equal the SAVE
     builds bit for bit (SAVE adds stores and ``ssp_with_grad``, which returns ``ssp<FAST>(x)`` itself: no operand order
     changes, and the library is compiled with -ffp-contract=off).
  B  mp_schnet_node_in_f32 against ``n = emb[z] W0 + b0 ; x = n Wx``: embedding widths 64 and 128, float32 and int64
     numbers, flags 2, 3, 66, 67, 67|512, with and without ``b0``, the counts of A and 33, numbers over the vocabulary,
     all equal, at both ends, outside it (a zero row: ``n`` is ``b0`` bit for bit), between two integers, out of range on
     the last row of a partial tile and on row 0, a vocabulary of 1.
  C  mp_schnet_stage0_f32 (node role and edge preparation in one launch) bit for bit against mp_edge_prepare_i64_f32 +
     mp_schnet_node_in_f32: the batches of test_gpu_schnet_tables.STAGE0_CASES, 4097 nodes with 300 edges, ``dist == NULL``,
     both sides of ``tiles16 > 1024`` and ``G > 1023``, no edges, no nodes, and its refusals.
  D  mp_schnet_node_residual_f32 (raw Keras kernels, ``keep_agg``, out of place), flags 0 and 1.
  E  mp_schnet_node_pack_f32 and mp_schnet_node_pack_bf16_f32 against the index formulas in the comments above the
     kernels and the three-way split stated at mp_bf16_piece_bits, and their refusals.

Every output buffer is filled with NaN and carries ``TAIL`` rows behind its logical end that must still be NaN afterwards;
buffers updated in place carry a tail of 7.0 that must be unchanged.  ``TAIL`` is one whole tile, so a kernel that lost
its row guard writes into the tail, not behind the buffer.  Every logical element is finite, every case compares once, and
every entry point runs twice on fresh buffers with bit-identical results.

Bars (none of its own): ``schnet_force_cases.BAR_CHAIN``, 2e-5 of the tensor's largest magnitude, against the float64
restatement, for every build; everything else is bitwise.

Distance of the float32 restatement from its float64 twin on these cases (NumPy, CPU; asserted at or below half the bar by
tests/test_schnet_node_cases.py, which prints each figure):

  MID / LAST n / x / h, N = 1 15 16 17 4080 4081 4097 8193, with biases   8.2e-08..3.8e-07 / 1.5e-07..6.3e-07 / 2.4e-07..7.0e-07
  MID / LAST n / x / h, N = 17 4081 4097 8193, every bias absent          2.0e-07..3.9e-07 / 3.5e-07..7.3e-07 / 3.6e-07..6.7e-07
  MID / LAST n / x / h, N = 37, pre-activations +-30                      3.1e-07 / 4.3e-07 / 5.2e-07
  input chain n / x, E = 64, N = 1 15 16 17 33 4081 4097 8193             <= 2.9e-07 / 5.1e-07 (every pattern, both vocabularies,
  input chain n / x, E = 128, the same counts                             <= 4.8e-07 / 5.5e-07  with and without b0)
  layer path n_out, N = 1 15 16 17 8193 / no biases 17 8193 / N = 37      8.2e-08..2.8e-07 / 2.0e-07..3.3e-07 / 3.1e-07

Largest distance of the kernels from the float64 restatement, measured on an MI355X with these tests (bar 2e-05):

  MID  n, x     flags 2 / 3 / 66 / 67 / 66|512 / 67|512    5.1e-07 / 4.9e-07 / 3.4e-07 / 3.1e-07 / 4.0e-07 / 3.3e-07
  LAST h        flags 2 / 3 / 66 / 67 / 66|512 / 67|512    6.7e-07 / 6.7e-07 / 4.5e-07 / 3.8e-07 / 4.5e-07 / 3.8e-07
  IN   n, x     flags 2, 3 / 66, 67, 67|512                5.5e-07 / 3.2e-07 (both widths, both number types)
  UPD  n_out    flags 0 / 1                                3.3e-07 / 3.3e-07
"""
import numpy as np
import pytest
import torch

import schnet_node_cases as C
from gcnn_keras_amd import _ffi
from test_gpu_schnet_tables import STAGE0_CASES

pytestmark = pytest.mark.gpu

TAIL = C.TILE     # rows behind the logical end of every buffer: one tile


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan(rows, *inner):
    return torch.full((rows + TAIL,) + inner, float("nan"), dtype=torch.float32, device="cuda")


def _held(a, value=7.0):
    """Device copy of ``a`` (rows, ...) with TAIL rows of ``value`` behind it: a buffer the kernel may update in place."""
    tail = np.full((TAIL,) + a.shape[1:], value, np.float32)
    return _dev(np.concatenate([a.astype(np.float32), tail], axis=0))


def _bits(a, b):
    """Bit for bit, NaN included."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _same_runs(first, second, what):
    for k in first:
        assert _bits(first[k], second[k]), "%s: %s differs between two runs" % (what, k)


def _all_nan(buf):
    return bool(torch.isnan(buf).all())


def _tail_is_nan(buf, rows, what):
    assert _all_nan(buf[rows:]), "%s: a store past row %d" % (what, rows)


def _tail_is_held(buf, rows, what):
    assert bool((buf[rows:] == 7.0).all()), "%s: a store past row %d" % (what, rows)


def _close(got, want, what):
    got = got.detach().double().cpu().numpy()
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.all(np.isfinite(got)), "%s: %d elements unwritten or not finite" % (what, int(np.sum(~np.isfinite(got))))
    err = C.max_rel(got, want)
    print("[node edges] %s: %.2e of the largest magnitude from float64 (bar %.0e)" % (what, err, C.BAR_CHAIN))
    if err > C.BAR_CHAIN:
        bad = np.argwhere(np.abs(got - want) > C.BAR_CHAIN * np.abs(want).max())
        print("[node edges] %s: %d elements off, rows %s, columns %s" % (what, len(bad), sorted(set(bad[:, 0]))[:20],
                                                                        sorted(set(bad[:, 1]))[:20]))
    assert err <= C.BAR_CHAIN, "%s: off by %.3g of the largest magnitude %.3g (bar %.1g)" % (what, err,
                                                                                           np.abs(want).max(), C.BAR_CHAIN)


def _pack(w, bf=False):
    """mp_schnet_node_pack_f32 / mp_schnet_node_pack_bf16_f32 image of a (K, U) matrix."""
    w = _dev(w)
    out = torch.empty(w.numel() * (3 if bf else 2) // 2, dtype=torch.float32, device="cuda")
    _ffi.call("mp_schnet_node_pack_bf16_f32" if bf else "mp_schnet_node_pack_f32", _ffi.ptr(w), int(w.shape[0]),
              int(w.shape[1]), _ffi.ptr(out), _ffi.stream())
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------- A. MID and LAST, inference builds
def _chain_buffers(c):
    n = c["N"]
    return {"agg": _held(c["agg"]), "n": _held(c["n"]), "x": _nan(n, C.F), "h": _nan(n, C.H)}


def _mid(c, img, bias, bufs, flags):
    _ffi.call("mp_schnet_node_update_f32", _ffi.ptr(bufs["agg"]), c["N"], _ffi.ptr(img["W2"]), _ffi.ptr(bias["b2"]),
              _ffi.ptr(img["W3"]), _ffi.ptr(bias["b3"]), _ffi.ptr(bufs["n"]), _ffi.ptr(img["Wx"]), _ffi.ptr(bufs["x"]),
              flags, _ffi.stream())
    torch.cuda.synchronize()


def _last(c, img, bias, bufs, flags):
    _ffi.call("mp_schnet_node_last_f32", _ffi.ptr(bufs["agg"]), c["N"], _ffi.ptr(img["W2"]), _ffi.ptr(bias["b2"]),
              _ffi.ptr(img["W3"]), _ffi.ptr(bias["b3"]), _ffi.ptr(bufs["n"]), _ffi.ptr(img["Wl0"]), _ffi.ptr(bias["bl0"]),
              _ffi.ptr(img["Wl1"]), _ffi.ptr(bias["bl1"]), _ffi.ptr(bufs["h"]), flags, _ffi.stream())
    torch.cuda.synchronize()


def _mid_save(c, img, bias, bufs, flags):
    bufs["d2"] = _nan(c["N"], C.F)
    _ffi.call("mp_schnet_node_update_save_f32", _ffi.ptr(bufs["agg"]), c["N"], _ffi.ptr(img["W2"]), _ffi.ptr(bias["b2"]),
              _ffi.ptr(img["W3"]), _ffi.ptr(bias["b3"]), _ffi.ptr(bufs["n"]), _ffi.ptr(img["Wx"]), _ffi.ptr(bufs["x"]),
              _ffi.ptr(bufs["d2"]), flags, _ffi.stream())
    torch.cuda.synchronize()


def _last_save(c, img, bias, bufs, flags):
    bufs.update(d2=_nan(c["N"], C.F), dl0=_nan(c["N"], C.F), dl1=_nan(c["N"], C.H))
    _ffi.call("mp_schnet_node_last_save_f32", _ffi.ptr(bufs["agg"]), c["N"], _ffi.ptr(img["W2"]), _ffi.ptr(bias["b2"]),
              _ffi.ptr(img["W3"]), _ffi.ptr(bias["b3"]), _ffi.ptr(bufs["n"]), _ffi.ptr(img["Wl0"]), _ffi.ptr(bias["bl0"]),
              _ffi.ptr(img["Wl1"]), _ffi.ptr(bias["bl1"]), _ffi.ptr(bufs["h"]), _ffi.ptr(bufs["d2"]), _ffi.ptr(bufs["dl0"]),
              _ffi.ptr(bufs["dl1"]), flags, _ffi.stream())
    torch.cuda.synchronize()


def _run(entry, c, img, bias, flags):
    bufs = _chain_buffers(c)
    entry(c, img, bias, bufs, flags)
    return bufs


CHAIN_RUNS = [(flags,) + run for flags in C.CHAIN_FLAGS for run in C.chain_runs(flags)]


@pytest.mark.parametrize("flags,n,bias,saturated", CHAIN_RUNS)
def test_mid_and_last_inference_builds(flags, n, bias, saturated):
    c = C.node_case(n, bias=bias, saturated=saturated)
    bf = bool(flags & C.BF)
    img = {k: _pack(c[k], bf) for k in ("W2", "W3", "Wx", "Wl0", "Wl1")}
    b = {k: _dev(c[k]) for k in ("b2", "b3", "bl0", "bl1")}
    want = C.node_restate(c, np.float64)
    tag = "N=%d flags=%d%s%s" % (n, flags, "" if bias else " no bias", " saturated" if saturated else "")
    n_in = _dev(c["n"])
    for chain, entry, save in (("MID", _mid, _mid_save), ("LAST", _last, _last_save)):
        what = "%s %s" % (chain, tag)
        bufs = _run(entry, c, img, b, flags)
        _same_runs(bufs, _run(entry, c, img, b, flags), what)
        if chain == "MID":
            _close(bufs["n"][:n], want["n"], what + " n")
            _close(bufs["x"][:n], want["x"], what + " x")
            _tail_is_nan(bufs["x"], n, what + " x")
            assert _all_nan(bufs["h"]), what + ": h belongs to the LAST chain"
        else:
            _close(bufs["h"][:n], want["h"], what + " h")
            _tail_is_nan(bufs["h"], n, what + " h")
            assert torch.equal(bufs["n"][:n], n_in), what + ": LAST reads the node state only"
            assert _all_nan(bufs["x"]), what + ": x belongs to the MID chain"
        assert not bool(bufs["agg"][:n].any()), what + ": consumed agg rows are zero again"
        _tail_is_held(bufs["agg"], n, what + " agg")
        _tail_is_held(bufs["n"], n, what + " n")
        if flags & C.HALF:                          # only the grid differs
            _same_runs(bufs, _run(entry, c, img, b, flags & ~C.HALF), what + ", half grid against full grid")
        if not bf:                                  # the SAVE build changes no operand order
            saved = _run(save, c, img, b, flags)
            for k in ("agg", "n", "x", "h"):
                assert _bits(bufs[k], saved[k]), "%s: %s differs from the SAVE build" % (what, k)


def test_mid_and_last_refuse_raw_kernels_and_run_nothing_on_no_nodes():
    c = C.node_case(17)
    img = {k: _pack(c[k]) for k in ("W2", "W3", "Wx", "Wl0", "Wl1")}
    b = {k: _dev(c[k]) for k in ("b2", "b3", "bl0", "bl1")}
    bufs = _chain_buffers(c)
    before = {k: v.clone() for k, v in bufs.items()}
    for entry in (_mid, _last):
        for flags in (0, 1, C.BF):
            with pytest.raises(ValueError):
                entry(c, img, b, bufs, flags)
        entry(dict(c, N=0), img, b, bufs, 3)
    _same_runs(before, bufs, "refused or empty")


# ------------------------------------------------------------------------------------- B. input chain
def _in_images(w, flags):
    bf = bool(flags & C.BF)
    return {"emb": _dev(w["emb"]), "W0": _pack(w["W0"], bf), "Wx": _pack(w["Wx"], bf), "b0": _dev(w["b0"])}


def _node_in(c, t, flags, numbers=None, n=None, emb_dim=None):
    rows = c["N"]
    bufs = {"n": _nan(rows, C.F), "x": _nan(rows, C.F)}
    numbers = _dev(c["numbers"]) if numbers is None else numbers
    _ffi.call("mp_schnet_node_in_f32", _ffi.ptr(numbers), rows if n is None else n, _ffi.ptr(t["emb"]), c["vocab"],
              c["emb_dim"] if emb_dim is None else emb_dim, _ffi.ptr(t["W0"]),
              _ffi.ptr(t["b0"]) if c["b0"] is not None else None, _ffi.ptr(t["Wx"]), _ffi.ptr(bufs["n"]),
              _ffi.ptr(bufs["x"]), flags | (C.I64 if c["i64"] else 0), _ffi.stream())
    torch.cuda.synchronize()
    return bufs


@pytest.mark.parametrize("flags", C.IN_FLAGS)
@pytest.mark.parametrize("i64", [False, True], ids=["float32", "int64"])
@pytest.mark.parametrize("emb_dim", [64, 128])
def test_input_chain(emb_dim, i64, flags):
    images = {vocab: _in_images(C.in_weights(emb_dim, vocab), flags) for vocab in (C.VOCAB, 1)}
    worst = {"n": 0.0, "x": 0.0}
    for bias in (True, False):
        for n, pattern, vocab in C.in_runs(flags, i64):
            c = C.in_case(n, emb_dim, pattern, vocab, bias=bias, i64=i64)
            t = images[vocab]
            what = "IN E=%d %s flags=%d N=%d %s vocab=%d%s" % (emb_dim, "int64" if i64 else "float32", flags, n, pattern,
                                                              vocab, "" if bias else " no bias")
            bufs = _node_in(c, t, flags)
            _same_runs(bufs, _node_in(c, t, flags), what)
            want = C.in_restate(c, np.float64)
            _, valid = C.in_rows(c)
            for k in ("n", "x"):
                _tail_is_nan(bufs[k], n, what + " " + k)
                if np.abs(want[k]).max() == 0:                    # every row out of range and no bias
                    assert not bool(bufs[k][:n].any()), what + " " + k
                    continue
                _close(bufs[k][:n], want[k], what + " " + k)
                worst[k] = max(worst[k], C.max_rel(bufs[k][:n].double().cpu().numpy(), want[k]))
            if (~valid).any():                                    # a zero embedding row: n is b0 bit for bit
                got = bufs["n"][:n][_dev(~valid)]
                row = t["b0"] if bias else torch.zeros(C.F, device="cuda")
                assert torch.equal(got, row.expand_as(got)), what + ": out-of-range numbers read a zero row"
            if flags & C.HALF:
                _same_runs(bufs, _node_in(c, t, flags & ~C.HALF), what + ", half grid against full grid")
    print("[node edges] IN E=%d %s flags=%d: largest n %.2e, x %.2e" % (emb_dim, "int64" if i64 else "float32", flags,
                                                                       worst["n"], worst["x"]))


def test_input_chain_refusals_and_no_nodes():
    c = C.in_case(17, 64)
    t = _in_images(c, 3)
    for kw in (dict(flags=1), dict(flags=0), dict(flags=3, emb_dim=32), dict(flags=3, n=-1)):
        flags = kw.pop("flags")
        with pytest.raises(ValueError):
            _node_in(c, t, flags, **kw)
    bufs = _node_in(c, t, 3, n=0)
    assert _all_nan(bufs["n"]) and _all_nan(bufs["x"])


# ------------------------------------------------------------------------------------- C. stage 0, chain variant
def _resident(b):
    # (an empty tensor has a null data pointer, which reads as "no coordinates": a batch without nodes hands in one row)
    xyz = b["node_coordinates"] if len(b["node_coordinates"]) else np.zeros((1, 3), np.float32)
    return {"z": _dev(b["node_number"]), "xyz": _dev(xyz), "idx": _dev(b["edge_indices"]),
            "ns": _dev(b["node_splits"]), "es": _dev(b["edge_splits"])}


def _stage0_buffers(n, m):
    return {"recv": torch.full((m + TAIL,), -3, dtype=torch.int32, device="cuda"),
            "send": torch.full((m + TAIL,), -3, dtype=torch.int32, device="cuda"), "dist": _nan(m),
            "flags": torch.zeros(1, dtype=torch.int32, device="cuda"), "n": _nan(n, C.F), "x": _nan(n, C.F)}


def _sizes(r):
    return int(r["z"].shape[0]), int(r["idx"].shape[0]), int(r["ns"].shape[0]) - 1


def _stage0_into(o, w, t, r, flags, with_dist=True, with_xyz=True, emb_dim=None):
    n, m, g = _sizes(r)
    try:
        _ffi.call("mp_schnet_stage0_f32", _ffi.ptr(r["z"]), n, _ffi.ptr(t["emb"]), w["vocab"],
                  w["emb_dim"] if emb_dim is None else emb_dim, _ffi.ptr(t["W0"]), _ffi.ptr(t["b0"]), _ffi.ptr(t["Wx"]),
                  _ffi.ptr(o["n"]), _ffi.ptr(o["x"]), _ffi.ptr(r["idx"]), m, _ffi.ptr(r["ns"]), _ffi.ptr(r["es"]), g,
                  _ffi.ptr(r["xyz"]) if with_xyz else None, _ffi.ptr(o["recv"]), _ffi.ptr(o["send"]),
                  _ffi.ptr(o["dist"]) if with_dist else None, _ffi.ptr(o["flags"]), flags, _ffi.stream())
    finally:
        torch.cuda.synchronize()


def _stage0(w, t, r, flags, with_dist=True, with_xyz=True):
    o = _stage0_buffers(*_sizes(r)[:2])
    _stage0_into(o, w, t, r, flags, with_dist, with_xyz)
    return o


def _two_launches(w, t, r, flags, with_dist=True, with_xyz=True):
    n, m, g = _sizes(r)
    o = _stage0_buffers(n, m)
    _ffi.call("mp_edge_prepare_i64_f32", _ffi.ptr(r["idx"]), m, _ffi.ptr(r["ns"]), _ffi.ptr(r["es"]), g, n,
              _ffi.ptr(r["xyz"]) if with_xyz else None, _ffi.ptr(o["recv"]), _ffi.ptr(o["send"]),
              _ffi.ptr(o["dist"]) if with_dist else None, _ffi.ptr(o["flags"]), _ffi.stream())
    _ffi.call("mp_schnet_node_in_f32", _ffi.ptr(r["z"]), n, _ffi.ptr(t["emb"]), w["vocab"], w["emb_dim"], _ffi.ptr(t["W0"]),
              _ffi.ptr(t["b0"]), _ffi.ptr(t["Wx"]), _ffi.ptr(o["n"]), _ffi.ptr(o["x"]), flags, _ffi.stream())
    torch.cuda.synchronize()
    return o


def _stage0_untouched(o, keys, what):
    for k in keys:
        if k in ("recv", "send"):
            assert bool((o[k] == -3).all()), "%s: %s written" % (what, k)
        elif k == "flags":
            assert int(o[k].item()) == 0, what
        else:
            assert _all_nan(o[k]), "%s: %s written" % (what, k)


def _stage0_flag_sets(n):
    out = list(C.STAGE0_FLAGS)
    if C.cap_of(C.STAGE0_FLAGS[1] | C.HALF, n) != C.cap_of(C.STAGE0_FLAGS[1], n):
        out.append(C.STAGE0_FLAGS[1] | C.HALF)
    return out


def _stage0_batches():
    out = {name: (build, None) for name, build in STAGE0_CASES.items()}
    out.update(C.stage0_cases())
    return out


DIST_NULL_CASES = ("six_graphs", "many_edges", "second-tile", "graphs-1024", "tiles-1025")   # both sides of the fallback


@pytest.mark.parametrize("emb_dim", [64, 128])
@pytest.mark.parametrize("case", list(_stage0_batches()))
def test_stage0_equals_edge_prepare_and_the_input_chain(case, emb_dim):
    build, fused = _stage0_batches()[case]
    b = build()
    r = _resident(b)
    n, m, g = _sizes(r)
    if fused is not None:
        assert C.stage0_fused(n, m, g) == fused, case
    if case.startswith("many_edges"):                  # the eight-wave launch keeps 64 edge workgroups
        assert C.stage0_fused(n, m, g) and C.stage0_edge_blocks_bf(m)[0] > C.stage0_edge_blocks_bf(m)[1] == 64
    w = C.in_weights(emb_dim)
    for flags in _stage0_flag_sets(n):
        t = _in_images(w, flags)
        what = "stage 0 %s E=%d flags=%d" % (case, emb_dim, flags)
        variants = [(True, True)]
        if case in DIST_NULL_CASES:                    # dist == NULL with and without coordinates
            variants += [(False, True), (False, False)]
        for with_dist, with_xyz in variants:
            got = _stage0(w, t, r, flags, with_dist, with_xyz)
            _same_runs(got, _stage0(w, t, r, flags, with_dist, with_xyz), what)
            ref = _two_launches(w, t, r, flags, with_dist, with_xyz)
            for k in ("recv", "send", "dist", "flags", "n", "x"):
                assert _bits(got[k], ref[k]), "%s%s: %s differs from the two launches" % (what, "" if with_dist else
                                                                                      " without dist", k)
            if n:
                assert bool(torch.isfinite(got["n"][:n]).all()) and bool(torch.isfinite(got["x"][:n]).all()), what
                _tail_is_nan(got["n"], n, what + " n")
                _tail_is_nan(got["x"], n, what + " x")
            else:
                _stage0_untouched(got, ("recv", "send", "dist", "flags", "n", "x"), what + ", no nodes")
            if m:
                assert bool((got["recv"][m:] == -3).all()) and bool((got["send"][m:] == -3).all()), what
                assert bool((got["recv"][:m] >= 0).all()) and bool((got["send"][:m] < n).all()), what
                if with_dist:
                    assert bool(torch.isfinite(got["dist"][:m]).all()), what
                    _tail_is_nan(got["dist"], m, what + " dist")
                else:
                    assert _all_nan(got["dist"]), what + ": dist written though not asked for"
            else:
                _stage0_untouched(got, ("recv", "send", "dist", "flags"), what + ", no edges")


def test_stage0_refusals_leave_every_buffer_alone():
    """``dist`` without coordinates, flags without bit 1 (packed images), an embedding width of 32 - on the fused side, and
    the first also where the call falls back to two launches (1024 single-node graphs)."""
    w = C.in_weights(64)
    everything = ("recv", "send", "dist", "flags", "n", "x")
    for case, build in (("six_graphs", STAGE0_CASES["six_graphs"]), ("graphs-1024", C.stage0_cases()["graphs-1024"][0])):
        r = _resident(build())
        n, m, g = _sizes(r)
        assert C.stage0_fused(n, m, g) == (case == "six_graphs")
        for flags in C.STAGE0_FLAGS:
            t = _in_images(w, flags)
            for kw in (dict(flags=flags, with_xyz=False), dict(flags=flags & ~C.PACKED), dict(flags=flags, emb_dim=32)):
                o = _stage0_buffers(n, m)
                with pytest.raises(ValueError):
                    _stage0_into(o, w, t, r, **kw)
                _stage0_untouched(o, everything, "refused stage 0 %s %s" % (case, kw))


# ------------------------------------------------------------------------------------- D. layer-path build
def _residual(c, b, flags):
    n = c["N"]
    bufs = {"agg": _held(c["agg"]), "n": _held(c["n"]), "n_out": _nan(n, C.F)}
    raw = {k: _dev(c[k]) for k in ("W2", "W3")}
    _ffi.call("mp_schnet_node_residual_f32", _ffi.ptr(bufs["agg"]), n, _ffi.ptr(raw["W2"]), _ffi.ptr(b["b2"]),
              _ffi.ptr(raw["W3"]), _ffi.ptr(b["b3"]), _ffi.ptr(bufs["n"]), _ffi.ptr(bufs["n_out"]), flags, _ffi.stream())
    torch.cuda.synchronize()
    return bufs


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("n,bias,saturated", C.RESIDUAL_RUNS)
def test_layer_path_build_on_raw_kernels(n, bias, saturated, flags):
    c = C.node_case(n, bias=bias, saturated=saturated)
    b = {k: _dev(c[k]) for k in ("b2", "b3")}
    what = "UPD N=%d flags=%d%s%s" % (n, flags, "" if bias else " no bias", " saturated" if saturated else "")
    bufs = _residual(c, b, flags)
    _same_runs(bufs, _residual(c, b, flags), what)
    _close(bufs["n_out"][:n], C.residual_restate(c, np.float64), what + " n_out")
    _tail_is_nan(bufs["n_out"], n, what + " n_out")
    assert _bits(bufs["agg"], _held(c["agg"])), what + ": keep_agg - the aggregation rows belong to the caller"
    assert _bits(bufs["n"], _held(c["n"])), what + ": out of place"


# ------------------------------------------------------------------------------------- E. pack kernels
def _pack_into(entry, w, k, u, out):
    _ffi.call(entry, _ffi.ptr(w), k, u, _ffi.ptr(out), _ffi.stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize("k,u", C.PACK_SHAPES)
def test_pack_kernels_write_the_stated_images(k, u):
    w = C.pack_weights(k, u)
    wd = _dev(w)
    images = []
    for _ in range(2):
        out = torch.full((k * u + TAIL,), float("nan"), device="cuda")
        _pack_into("mp_schnet_node_pack_f32", wd, k, u, out)
        images.append(out)
    assert _bits(images[0], images[1])
    assert _all_nan(images[0][k * u:]), "mp_schnet_node_pack_f32 %dx%d: a store past the image" % (k, u)
    got = images[0][:k * u].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), C.pack_restate(w).view(np.uint32)), "FP32 image %dx%d" % (k, u)
    assert np.array_equal(np.sort(got), np.sort(w.reshape(-1)))                    # a permutation of W

    dwords = k * u * 3 // 2
    images = []
    for _ in range(2):
        out = torch.full((dwords + TAIL,), float("nan"), device="cuda")
        _pack_into("mp_schnet_node_pack_bf16_f32", wd, k, u, out)
        images.append(out)
    assert _bits(images[0], images[1])
    assert _all_nan(images[0][dwords:]), "mp_schnet_node_pack_bf16_f32 %dx%d: a store past the image" % (k, u)
    halves = images[0][:dwords].cpu().numpy().view(np.uint16)
    bits, values = C.bf16_split(w)
    pieces = C.pack_bf16_decode(halves, k, u)
    for pc, name in enumerate(("hi", "mid", "lo")):
        assert np.array_equal(pieces[pc].view(np.uint32) >> 16, bits[pc].astype(np.uint32)), \
            "bf16 image %dx%d: piece %s" % (k, u, name)
    total = pieces[0].astype(np.float64) + pieces[1].astype(np.float64) + pieces[2].astype(np.float64)
    assert np.array_equal(total, w.astype(np.float64)), "bf16 image %dx%d: hi + mid + lo != W" % (k, u)
    assert np.array_equal(halves, C.pack_bf16_restate(w))


def test_pack_kernels_refuse_shapes_off_their_tiles():
    wd = _dev(C.pack_weights(128, 128))
    out = torch.full((3 * 128 * 128 // 2,), float("nan"), device="cuda")
    for entry, k, u in (("mp_schnet_node_pack_f32", 24, 128), ("mp_schnet_node_pack_bf16_f32", 24, 128),
                        ("mp_schnet_node_pack_bf16_f32", 48, 128), ("mp_schnet_node_pack_f32", 64, 96),
                        ("mp_schnet_node_pack_bf16_f32", 64, 96), ("mp_schnet_node_pack_f32", 0, 128)):
        with pytest.raises(ValueError):
            _pack_into(entry, wd, k, u, out)
    torch.cuda.synchronize()
    assert _all_nan(out)
    _pack_into("mp_schnet_node_pack_f32", wd, 48, 128, out)        # K = 48 is a shape of the FP32 packer
    assert bool(torch.isfinite(out[:48 * 128]).all()) and _all_nan(out[48 * 128:])
