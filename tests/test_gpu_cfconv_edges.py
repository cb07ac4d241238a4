"""The fused continuous-filter convolution (csrc/mp_cfconv.hip) off the molecular shapes, through the C ABI against the
float32 and float64 restatements of tests/cfconv_cases.py: every wave-uniform tile shape of the segment walk with segments
that stay inside a tile and segments that run through 30 whole tiles, sorted and through ``perm``; edge counts around the
tile, the workgroup and every small grid size; the second trip of the 4-wave and the 8-wave build and two tiles per wave
under the half grid; the basis sizes on either side of the fixed builds on both entry points; absent biases, an offset, a
narrow basis, distances at 0 and far outside the basis, saturated pre-activations; the deterministic mode against itself
(two runs, a side stream, another grid) and against the default mode; the layer on both modes; the pack image bit by bit.

Every run hands the kernel ``out`` with its N rows zero and five rows of NaN behind them that must still be NaN
afterwards; receivers without edges must be exactly 0; in deterministic mode the workspace carries 256 bytes of a fixed
pattern behind its end that must be unchanged.  Every case compares once, with ``parity.assert_rows_close`` at its defaults
(1e-5 per row against the float32 restatement, the float64 twin given) and nothing else.

Distance of the float32 restatement from its float64 twin (``parity.rowwise_rel``, NumPy, CPU; asserted at or below 5e-6 by
tests/test_cfconv_cases.py, which prints each figure):

  layout graph (80 tiles of prescribed patterns), sorted / shuffled          5.9e-07 / 7.1e-07
  unaligned graph (601 receivers of 1..1000 edges), sorted / shuffled        9.2e-07 / 9.1e-07
  exact M = 1 31 32 33 127 128 129 255 256 257 (5 nodes)                     1.4e-07..4.7e-07
  M = 128 g - 5, g = 1..17 (5 nodes: up to 434 edges per receiver)           3.7e-07..3.4e-06
  32 801 edges over 40 nodes / 65 569 over 80 / 257, 1333 over 40            2.5e-06 / 2.4e-06 / 5.9e-07, 4.0e-07
  B = 1 2 19 20 21 24 25 26 30 31 32 on 400 edges, Gauss / given basis       3.4e-07..5.7e-07 / 3.2e-07..5.6e-07
  no b1, no b2, neither, offset 0.75, sigma 0.1 with 32 bins                 3.0e-07..5.2e-07
  d = 0, d = 3 x distance, |pre-activation| up to 100                        3.4e-07, 3.4e-07, 3.6e-07
  layer cases (given basis): 25 bins, shuffled unaligned graph / no biases   1.0e-06 / 6.5e-07
"""
import numpy as np
import pytest
import torch

import cfconv_cases as C
import topologies as T
from gcnn_keras_amd import _ffi
from gcnn_keras_amd.ragged import RaggedTensor
from parity import assert_rows_close, rowwise_rel

pytestmark = pytest.mark.gpu

TAIL = 5          # rows of NaN behind the N rows of ``out``
WS_TAIL = 256     # bytes of a fixed pattern behind the deterministic mode's workspace
_DEVICE = {}


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).cuda()      # (a copy: the cases are read-only)


def _pack(c, bins=None):
    packed = torch.full((_ffi.lib().mp_cfconv_packed_floats(),), float("nan"), dtype=torch.float32, device="cuda")
    t = [_dev(c[k]) for k in ("w1", "b1", "w2", "b2")]
    _ffi.call("mp_cfconv_pack_f32", _ffi.ptr(t[0]), _ffi.ptr(t[1]), c["bins"] if bins is None else bins, _ffi.ptr(t[2]),
              _ffi.ptr(t[3]), _ffi.ptr(packed), _ffi.stream())
    torch.cuda.synchronize()
    return packed


def _operands(name):
    """Device copies of a case's operands, made once: the receivers ascending, ``perm`` where the list is not sorted,
    senders and distances in list order, the packed weights."""
    if name not in _DEVICE:
        c = C.get(name)
        recv_sorted, perm = C.kernel_order(c)
        _DEVICE[name] = {"x": _dev(c["x"]), "dist": _dev(c["dist"]), "recv": _dev(recv_sorted), "send": _dev(c["send"]),
                         "perm": _dev(perm), "packed": _pack(c)}
    return _DEVICE[name]


def _rbf(name):
    t = _operands(name)
    if "rbf" not in t:
        t["rbf"] = _dev(C.given_rbf(C.get(name)))
    return t["rbf"]


def _ws_pattern():
    return ((torch.arange(WS_TAIL, device="cuda") * 7 + 3) % 251).to(torch.uint8)


def _launch(name, flags, entry="gauss"):
    """One call of the entry point (``entry`` "gauss" / "rbf"; flag bit 5 selects the workspace variant) on a fresh ``out``;
    returns the N rows after the checks every run shares."""
    c, t = C.get(name), _operands(name)
    n, m, bins = c["N"], c["M"], c["bins"]
    out = torch.full((n + TAIL, C.F), float("nan"), dtype=torch.float32, device="cuda")
    out[:n] = 0.0
    edge = [_ffi.ptr(t["dist"]), bins, c["distance"], c["sigma"], c["offset"]] if entry == "gauss" else \
        [_ffi.ptr(_rbf(name)), bins]
    head = [_ffi.ptr(t["x"]), n] + edge + [_ffi.ptr(t["packed"]), _ffi.ptr(t["recv"]), _ffi.ptr(t["send"]),
                                           _ffi.ptr(t["perm"]), m, flags, _ffi.ptr(out)]
    fn = "mp_cfconv_gauss_fused" if entry == "gauss" else "mp_cfconv_fused"
    if flags & 32:
        nbytes = _ffi.workspace_bytes("mp_cfconv_det_workspace_bytes", m)
        ws = torch.full((nbytes + WS_TAIL,), 0xA5, dtype=torch.uint8, device="cuda")
        ws[nbytes:] = _ws_pattern()
        _ffi.call(fn + "_ws_f32", *head, _ffi.ptr(ws), nbytes, _ffi.stream())
    else:
        _ffi.call(fn + "_f32", *head, _ffi.stream())
    torch.cuda.synchronize()
    what = "%s flags %d (%s)" % (name, flags, entry)
    assert bool(torch.isnan(out[n:]).all()), "%s: a store past row %d" % (what, n)
    if flags & 32:
        assert torch.equal(ws[nbytes:], _ws_pattern()), "%s: a store past the workspace" % what
    return out[:n]


def _compare(family, name, got, flags, entry="gauss", route=""):
    """Receivers without edges exactly 0, everything finite, rows against both restatements (printed first)."""
    c = C.get(name)
    r32, r64 = C.restated(name, entry)
    got = got.detach().cpu().numpy()
    what = "%s flags %d (%s%s)" % (name, flags, entry, route)
    deg = np.bincount(c["recv"], minlength=c["N"])
    assert np.all(np.isfinite(got)), "%s: %d elements not finite" % (what, int(np.sum(~np.isfinite(got))))
    assert not got[deg == 0].any(), "%s: a receiver without edges is not 0" % what
    print("[cfconv] %-10s %-44s worst row %.2e from float32, %.2e from float64 (restatement %.2e)" % (
        family, what, rowwise_rel(got, r32), rowwise_rel(got, r64), rowwise_rel(r32, r64)))
    return assert_rows_close(got, r32, r64, what=what)


def _on_side_stream(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------ A, B, G: layouts
@pytest.mark.parametrize("flags", [0, 1, 5, 17])
@pytest.mark.parametrize("name", C.LAYOUT_CASES)
def test_layouts(name, flags):
    """Every tile shape of the segment walk - boundaries at each edge of a tile, 32 single-edge receivers, interior
    segments over edges 15|16, receivers ending on half and tile boundaries, segments through 30 whole tiles - sorted and
    through ``perm``, exact and fast softplus, 4 and 8 waves, the half grid."""
    _compare("layout", name, _launch(name, flags), flags)


@pytest.mark.parametrize("name", C.LAYOUT_CASES)
def test_layouts_deterministic(name):
    """Flag 32 on the same graphs: rows against the restatements; two runs and a run on a side stream give equal bits;
    flags 33 and 49 (the same build, another tile-to-wave mapping: slot order is tile order) give equal bits; where no
    receiver touches more than two tiles, the default mode gives the same bits (a + b == b + a)."""
    outs = {}
    for flags in (33, 37, 49):
        first = _launch(name, flags)
        _compare("layout-det", name, first, flags)
        assert torch.equal(first, _launch(name, flags)), "%s flags %d: two runs differ" % (name, flags)
        assert torch.equal(first, _on_side_stream(lambda: _launch(name, flags))), "%s flags %d: side stream" % (name, flags)
        outs[flags] = first
    assert torch.equal(outs[33], outs[49]), "%s: flags 33 and 49 differ" % name
    print("[cfconv] %s: flags 33 and 37 (4 and 8 waves) give %s bits" % (
        name, "equal" if torch.equal(outs[33], outs[37]) else "different"))
    c = C.get(name)
    e = np.stack([c["recv"], c["send"]], axis=-1).astype(np.int64)
    if T.tile_placement(e, c["N"])["max_tiles_touched"] <= 2:
        assert name.startswith("layout")
        assert torch.equal(outs[33], _launch(name, 1)), "%s: default and deterministic mode differ" % name
    else:
        assert name.startswith("unaligned")


# ------------------------------------------------------------------------------------------------ C, D: counts, grids, trips
@pytest.mark.parametrize("name", C.COUNT_CASES)
def test_edge_counts_and_grids(name):
    """M around the tile (32), the workgroup (128 / 256) and 128 g - 5 for g = 1..17 workgroups (the XCD block order at
    every remainder of 8, waves without a tile, the partial last tile), 4 waves, 8 waves and the half grid."""
    for flags in (1, 5, 17):
        _compare("counts", name, _launch(name, flags), flags)


@pytest.mark.parametrize("name", C.TRIP_CASES)
def test_trips(name):
    """The second trip of the persistent tile loop (prefetch across the trip, a receiver that owns the tiles on both
    sides): 32 801 edges on 256 x 4 waves, 65 569 on 256 x 8 (flags 5); two tiles per wave under the half grid at 257
    and 1333 edges; deterministic mode on all of them."""
    for flags in ((5,) if name == "trip8" else (1, 5, 17)):
        _compare("trips", name, _launch(name, flags), flags)
    det = _launch(name, 33)
    _compare("trips-det", name, det, 33)
    if name.startswith("half"):
        assert torch.equal(det, _launch(name, 49)), "%s: flags 33 and 49 differ" % name


# ------------------------------------------------------------------------------------------------ E: bases
@pytest.mark.parametrize("entry", ["gauss", "rbf"])
@pytest.mark.parametrize("name", C.BASIS_CASES)
def test_bases(name, entry):
    """B = 1 2 19 20 21 24 25 26 30 31 32 (``nk = (B + 2) >> 1``: the generic build around the fixed builds of 20 and 25,
    odd and even row counts, the largest) from distances and from a given basis matrix, exact and fast softplus."""
    for flags in (0, 1):
        _compare("bases", name, _launch(name, flags, entry), flags, entry)


@pytest.mark.parametrize("bins", [0, 33])
def test_basis_bounds_are_refused_before_anything_is_written(bins):
    c = C.get("bins20")
    with pytest.raises(ValueError):
        _pack(c, bins=bins)
    packed = torch.full((_ffi.lib().mp_cfconv_packed_floats(),), float("nan"), dtype=torch.float32, device="cuda")
    w1, w2 = _dev(c["w1"]), _dev(c["w2"])
    assert _ffi.lib().mp_cfconv_pack_f32(_ffi.ptr(w1), None, bins, _ffi.ptr(w2), None, _ffi.ptr(packed),
                                         _ffi.stream()) == _ffi.MP_EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(packed).all())
    t = _operands("bins20")
    n, m = c["N"], c["M"]
    out = torch.full((n + TAIL, C.F), float("nan"), dtype=torch.float32, device="cuda")
    tail = [_ffi.ptr(t["packed"]), _ffi.ptr(t["recv"]), _ffi.ptr(t["send"]), None, m, 1, _ffi.ptr(out), _ffi.stream()]
    with pytest.raises(ValueError):
        _ffi.call("mp_cfconv_gauss_fused_f32", _ffi.ptr(t["x"]), n, _ffi.ptr(t["dist"]), bins, c["distance"], c["sigma"],
                  c["offset"], *tail)
    with pytest.raises(ValueError):
        _ffi.call("mp_cfconv_fused_f32", _ffi.ptr(t["x"]), n, _ffi.ptr(_rbf("bins20")), bins, *tail)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------------ F: parameters
@pytest.mark.parametrize("name", C.PARAMETER_CASES)
def test_parameters(name):
    """``b1`` absent, ``b2`` absent, both; offset 0.75; sigma 0.1 with 32 bins; distances exactly 0 and at 3 x
    ``distance``; first-layer weights scaled until the pre-activations reach +-100 - exact and fast softplus."""
    for flags in (0, 1):
        _compare("parameters", name, _launch(name, flags), flags)


def _layer(c, deterministic=False):
    from gcnn_keras_amd.layers.conv.schnet_conv import SchNetCFconv
    bias = c["b1"] is not None
    assert bias == (c["b2"] is not None)
    lay = SchNetCFconv(units=128, use_bias=bias)
    lay.ensure_built([(None, None, 128), (None, None, c["bins"]), (None, None, 2)])
    with torch.no_grad():
        lay.lay_dense1.kernel.copy_(_dev(c["w1"]))
        lay.lay_dense2.kernel.copy_(_dev(c["w2"]))
        if bias:
            lay.lay_dense1.bias.copy_(_dev(c["b1"]))
            lay.lay_dense2.bias.copy_(_dev(c["b2"]))
    assert (lay.lay_dense1.bias is None) == (not bias) and (lay.lay_dense2.bias is None) == (not bias)
    lay.deterministic = deterministic
    ns, es = np.array([0, c["N"]], np.int64), np.array([0, c["M"]], np.int64)
    inputs = [RaggedTensor.from_numpy(np.array(c["x"]), ns), RaggedTensor.from_numpy(C.given_rbf(c), es),
              RaggedTensor.from_numpy(np.stack([c["recv"], c["send"]], axis=-1).astype(np.int64), es)]
    return lay, inputs


def test_layer_without_biases_takes_the_fused_route():
    """``SchNetCFconv(units=128, use_bias=False)``: ``fused=True`` (both bias pointers null in the pack kernel) against
    ``fused=False`` (the layer sequence) and both against the restatement."""
    name = "layer-no-bias"
    lay, inputs = _layer(C.get(name))
    with torch.no_grad():
        fused = lay(inputs, fused=True).values
        layered = lay(inputs, fused=False).values
    torch.cuda.synchronize()
    _compare("layer", name, fused, 1, "rbf", ", fused layer")
    _compare("layer", name, layered, 0, "rbf", ", layer sequence")
    r64 = C.restated(name, "rbf")[1]
    assert_rows_close(fused.cpu().numpy(), layered.cpu().numpy(), r64, what="fused layer against the layer sequence")


def test_layer_deterministic_through_perm():
    """``SchNetCFconv`` with ``deterministic = True`` (flags 33 with a workspace, what the crystal builder sets) on the
    shuffled unaligned graph - receivers of up to 1000 edges, reached through ``perm`` - with an edge width of 25: equal
    bits over two calls, rows against the restatement."""
    name = "layer-det"
    lay, inputs = _layer(C.get(name), deterministic=True)
    with torch.no_grad():
        first = lay(inputs, fused=True).values
        second = lay(inputs, fused=True).values
    torch.cuda.synchronize()
    assert torch.equal(first, second)
    _compare("layer", name, first, 33, "rbf", ", deterministic layer")


# ------------------------------------------------------------------------------------------------ pack image
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("bins", [1, 20, 31, 32])
def test_pack_image(bins, bias):
    """mp_cfconv_pack_f32 bit by bit: the FP32 rows ``[k][4 c + blk] = W1[k][32 blk + c]`` with ``b1`` as row B and zero
    rows behind it, ``b2``, the three bf16 images of W2 (hi + mid + lo, summed in float64, within 2^-23 of the entry:
    three 8-bit pieces carry 24 significant bits, one more bit for the rounding of the last piece) and the bf16 images of
    W1 | b1 (the same bound; all zero at 32 bins, where ``nk`` = 17 > 16 - at 31 bins ``nk`` is 16 and the image is
    filled)."""
    c = dict(C.get("bins%d" % bins))
    if not bias:
        c["b1"] = c["b2"] = None
    image = _pack(c).cpu().numpy()
    assert image.shape == (C.PACKED_FLOATS,) and not np.isnan(image).any()
    rows = np.zeros((C.MAX_KROWS, C.F), np.float32)
    rows[:bins] = c["w1"]
    if bias:
        rows[bins] = c["b1"]
    want = rows.reshape(C.MAX_KROWS, 4, 32).transpose(0, 2, 1).reshape(C.MAX_KROWS, C.F)     # [k][4 c + blk]
    assert np.array_equal(image[:C.MAX_KROWS * C.F].view(np.uint32), want.reshape(-1).view(np.uint32))
    o = C.MAX_KROWS * C.F
    w2 = C.decode_w2_images(image[o:o + 3 * C.W2_PIECE_FLOATS])
    o += 3 * C.W2_PIECE_FLOATS
    b2 = c["b2"] if bias else np.zeros(C.F, np.float32)
    assert np.array_equal(image[o:o + C.F].view(np.uint32), b2.view(np.uint32))
    o += C.F
    entry = c["w2"].astype(np.float64)
    resid = np.abs(w2.sum(axis=0) - entry)
    print("[cfconv] pack B=%d: W2 pieces off by at most %.2e of the entry (2^-23 = %.2e)" % (
        bins, float(np.max(resid / np.abs(entry))), 2.0 ** -23))
    assert np.all(resid <= 2.0 ** -23 * np.abs(entry))
    w1b = image[o:]
    assert w1b.shape == (C.W1B_FLOATS,)
    if bins == 32:
        assert not w1b.view(np.uint32).any()
    else:
        pieces, unused = C.decode_w1_images(w1b, bins)
        assert unused == 0.0
        assert np.all(np.abs(pieces.sum(axis=0) - rows.astype(np.float64)) <= 2.0 ** -23 * np.abs(rows.astype(np.float64)))
