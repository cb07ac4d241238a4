"""INorp on the engine (literature/INorp.py, layers/conv/inorp_conv.py, csrc/mp_inorp.hip): the folded edge kernel and
its reverse against the torch restatement (tests/inorp_reference.py: float32 with the float64 twin as budget) on hand-made
lists around the 32-position tile; the step on both routes, with and without a tape; bits on a second call and a second
stream; the model eager and replayed, through ``predict``, in training and through ``fit``."""
import contextlib

import numpy as np
import pytest
import torch

import inorp_reference as ref
from gcnn_keras_amd import _ffi, synth
from gcnn_keras_amd.layers.conv.inorp_conv import EdgeStepSpec, INorpEdgeStep
from gcnn_keras_amd.literature import INorp
from gcnn_keras_amd.ragged import RaggedTensor
from parity import BAR_CAP, assert_rows_close, rowwise_rel

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
WIDTHS = [16, 32, 64, 128]         # H1: the kernel's four builds
EDGE_WIDTHS = [1, 8, 11, 32, 64]   # Fe: 1 and 11 are padded to the k step of 4, 64 is the widest


def _rag(values, splits):
    return RaggedTensor.from_numpy(np.ascontiguousarray(values), np.asarray(splits, np.int64))


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _vec(a):
    """A bias gradient as ONE row: each element is a sum over all rows that may cancel to any fraction of the vector's
    scale; the vector as a whole is what the optimizer applies (tests/test_gpu_dmpnn.py)."""
    a = np.asarray(a)
    return a.reshape(1, -1) if a.ndim == 1 else a


def _col(a):
    """``edges_bar`` at edge width 1 as ONE row, for the reason ``_vec`` gives: each of its rows is a single sum of H1
    signed products, so a row-wise relative bound would measure how far that sum cancels, in any float32 pipeline.  Wider
    gradients stay as they are."""
    a = np.asarray(a)
    return a.reshape(1, -1) if (a.ndim == 2 and a.shape[1] == 1) else a


def _show_rowwise(what, got, r32, r64):
    """The row-wise figure ``_col`` sets aside, printed beside the float32 restatement's own, so that it stays in sight."""
    if np.asarray(r64).ndim == 2 and np.asarray(r64).shape[1] == 1:
        print("[inorp] %s: one column, row-wise: engine %.2e, float32 restatement %.2e from float64"
              % (what, rowwise_rel(got, r64), rowwise_rel(r32, r64)))


@contextlib.contextmanager
def engine_calls():
    """The names of the engine calls issued inside, in order."""
    names, real = [], _ffi.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    _ffi.call = call
    try:
        yield names
    finally:
        _ffi.call = real


def _fused_only(names, steps=1, reverse=0):
    """The fused route ran ``steps`` times (``reverse`` times backwards) and wrote nothing edge-sized on its way."""
    assert names.count("mp_inorp_edge_f32") == steps and names.count("mp_inorp_edge_grad_f32") == reverse, names
    assert "mp_gather_rows_f32" not in names and not any("concat" in n for n in names), names


def _sequence_only(names):
    assert not any(n.startswith("mp_inorp") for n in names) and "mp_gather_rows_f32" in names, names


def _twice_bar(got, other, r32, r64, what):
    """Fused and layer sequence agree within twice the bar each of them is held to against the restatement."""
    bar = 2 * max(1e-5, min(2 * rowwise_rel(r32, r64), BAR_CAP))
    err = rowwise_rel(got, other)
    assert err <= bar, "%s: fused and layer sequence differ by %.3g (bar %.1g)" % (what, err, bar)


# ------------------------------------------------------------------------------------------------ the two kernels
def kernel_case(kind, h1, fe, seed=0):
    """Operands of the two kernels for the list ``kind``: random ``Pj``, ``Pi``, edge rows, ``Wc`` and upstream ``g``."""
    b = ref.edge_list(kind)
    rng = np.random.default_rng(seed + 5 * h1 + fe)
    n, m = int(b["node_splits"][-1]), int(b["edge_splits"][-1])
    ops = {"pj": 0.5 * rng.normal(size=(n, h1)), "pi": 0.5 * rng.normal(size=(n, h1)),
           "edges": 0.5 * rng.normal(size=(m, fe)), "wc": rng.uniform(-0.5, 0.5, size=(fe, h1)),
           "g": rng.normal(size=(n, h1))}
    return b, {k: v.astype(np.float32) for k, v in ops.items()}


def kernel_spec(b, edge_width, activation, method):
    ns, es = b["node_splits"], b["edge_splits"]
    nodes = _rag(np.zeros((int(ns[-1]), 1), np.float32), ns)
    edges = _rag(np.zeros((int(es[-1]), edge_width), np.float32), es)
    return EdgeStepSpec(nodes, edges, _rag(b["edge_indices"], es), activation, method)


def restated_kernels(b, ops, activation, method, dtype):
    recv, send = ref.flat_indices(b)
    t = {k: _t(v, dtype) for k, v in ops.items()}
    out = ref.edge_kernel(t["pj"], t["pi"], t["edges"], t["wc"], recv, send, activation, method)
    rev = ref.edge_kernel_reverse(t["pj"], t["pi"], t["edges"], t["wc"], recv, send, activation, method, t["g"])
    return [out.numpy()] + [x.numpy() for x in rev]


@pytest.mark.parametrize("method", ["segment_sum", "segment_mean"])
@pytest.mark.parametrize("h1", WIDTHS)
def test_kernels_on_hand_made_lists(h1, method):
    for kind in ref.EDGE_LISTS:
        for fe in EDGE_WIDTHS:
            activation = ref.ACTIVATIONS[(EDGE_WIDTHS.index(fe) + ref.EDGE_LISTS.index(kind)) % len(ref.ACTIVATIONS)]
            b, ops = kernel_case(kind, h1, fe)
            spec = kernel_spec(b, fe, activation, method)
            g = {k: _t(v, F32).cuda() for k, v in ops.items()}
            out = spec.forward(g["pj"], g["pi"], g["edges"], g["wc"])
            pj_bar, pi_bar, e_bar, wc_bar = spec.grad(g["pj"], g["pi"], g["edges"], g["wc"], g["g"], True, True, True)
            again = spec.forward(g["pj"], g["pi"], g["edges"], g["wc"])
            again_bar = spec.grad(g["pj"], g["pi"], g["edges"], g["wc"], g["g"], True, True, True)
            torch.cuda.synchronize()
            what = "INorp kernels %s H1=%d Fe=%d %s %s" % (kind, h1, fe, activation, method)
            assert torch.equal(_bits(out), _bits(again)), what
            for a, c in zip((pj_bar, pi_bar, e_bar, wc_bar), again_bar):
                assert torch.equal(_bits(a), _bits(c)), what
            r32, r64 = (restated_kernels(b, ops, activation, method, dt) for dt in (F32, F64))
            recv, _ = ref.flat_indices(b)
            received = np.zeros(out.shape[0], bool)
            received[recv.numpy()] = True
            assert not out.cpu().numpy()[~received].any(), what + ": a receiver without edges is exactly 0"
            assert not pi_bar.cpu().numpy()[~received].any(), what
            assert_rows_close(out.cpu().numpy(), r32[0], r64[0], what=what + ": out")
            if int(b["edge_splits"][-1]) == 0:
                assert not pj_bar.any() and not wc_bar.any() and tuple(e_bar.shape) == (0, fe)
                continue
            for name, got, k in (("Pi_bar", pi_bar, 2), ("Pj_bar", pj_bar, 3), ("Wc_bar", wc_bar, 4), ("edges_bar", e_bar, 5)):
                shape = _col if name == "edges_bar" else np.asarray
                if name == "edges_bar":
                    _show_rowwise(what, got.cpu().numpy(), r32[k], r64[k])
                assert_rows_close(shape(got.cpu().numpy()), shape(r32[k]), shape(r64[k]), what="%s: %s" % (what, name))


def _raw_grad(spec, g, h1):
    """``gz`` itself (``spec.grad`` consumes it): one direct call of the reverse kernel."""
    head, ws, nbytes, _ = spec._args(g["pj"], g["pi"], g["edges"], g["wc"])
    gz = torch.full((spec.e, h1), float("nan"), device="cuda")
    pi_bar = torch.full((spec.n, h1), float("nan"), device="cuda")
    _ffi.call("mp_inorp_edge_grad_f32", *head, _ffi.ptr(g["g"]), _ffi.ptr(ws), nbytes, _ffi.ptr(gz), _ffi.ptr(pi_bar),
              _ffi.stream())
    return gz, pi_bar


@pytest.mark.parametrize("method", ["segment_sum", "segment_mean"])
@pytest.mark.parametrize("kind", ["e33", "star70", "cut1", "batch8_shuffled"])
def test_reverse_kernel_writes_gz_at_list_positions(kind, method):
    """``gz`` lies at the edge's LIST position also where the list is unsorted; relu with exact zeros in ``z1`` takes the
    derivative 0 there, as ``mp_activation_grad_f32`` does."""
    h1, fe = 32, 8
    b, ops = kernel_case(kind, h1, fe, seed=3)
    recv, send = ref.flat_indices(b)
    # exact zeros in z1: every fourth edge has zero features, and the rows it gathers cancel in the first 8 columns
    ops["edges"][::4] = 0.0
    ops["pj"][:, :8] = 1.25
    ops["pi"][:, :8] = -1.25
    spec = kernel_spec(b, fe, "relu", method)
    g = {k: _t(v, F32).cuda() for k, v in ops.items()}
    gz, pi_bar = _raw_grad(spec, g, h1)
    r32, r64 = (restated_kernels(b, ops, "relu", method, dt) for dt in (F32, F64))
    z1 = (_t(ops["pj"], F32)[send] + _t(ops["pi"], F32)[recv]) + _t(ops["edges"], F32) @ _t(ops["wc"], F32)
    assert int((z1 == 0).sum()) >= 8 * ((len(recv) + 3) // 4)
    assert not gz.cpu()[z1 == 0].any()
    assert bool(torch.isfinite(gz).all()) and bool(torch.isfinite(pi_bar).all())
    what = "INorp gz %s %s" % (kind, method)
    assert_rows_close(gz.cpu().numpy(), r32[1], r64[1], what=what)
    assert_rows_close(pi_bar.cpu().numpy(), r32[2], r64[2], what=what + ": Pi_bar")
    # the derivative of relu at an exact zero, against the standalone kernel
    pre, gy = z1.cuda().contiguous(), torch.ones_like(z1).cuda()
    want = torch.empty_like(pre)
    _ffi.call("mp_activation_grad_f32", _ffi.MP_ACT_RELU, 0.05, _ffi.ptr(pre), _ffi.ptr(gy), pre.numel(), _ffi.ptr(want),
              _ffi.stream())
    assert torch.equal(want.cpu() != 0, z1 > 0)


@pytest.mark.parametrize("h1", [32, 128])
def test_kernels_are_deterministic_across_streams(h1):
    b, ops = kernel_case("batch8_shuffled", h1, 11, seed=5)
    spec = kernel_spec(b, 11, "swish", "segment_mean")
    g = {k: _t(v, F32).cuda() for k, v in ops.items()}

    def run():
        out = spec.forward(g["pj"], g["pi"], g["edges"], g["wc"])
        return (out,) + _raw_grad(spec, g, h1)
    first = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        second = run()
    side.synchronize()
    for name, a, c in zip(("out", "gz", "Pi_bar"), first, second):
        assert torch.equal(_bits(a), _bits(c)), name


@pytest.mark.parametrize("method", ["sum", "mean"])
def test_kernel_skips_indices_out_of_range(method):
    """Direct calls on a hand-built plan, outputs filled with NaN: an edge whose sender lies outside [0, N) adds an exact 0
    wherever it stands in its receiver's range - here in the middle of one, and as the only edge of another receiver, which
    must come out as 0 - reads nothing and gets a zero row of ``gz``; the mean divides by the range's length.  Edges whose
    receiver lies outside lie behind the last range."""
    n, h1, fe = 6, 16, 3
    recv = np.array([0, 0, 1, 1, 1, 3, 3, 4, 9, -2], np.int32)     # sorted positions; the last two receivers are outside
    send = np.array([2, 5, 4, 77, 1, 0, 2, -1, 1, 3], np.int32)    # position 3: mid-range; position 7: receiver 4's only edge
    valid = (recv >= 0) & (recv < n) & (send >= 0) & (send < n)
    ptr0 = np.array([0, 2, 5, 5, 7, 8, 8], np.int32)
    e = len(recv)
    rng = np.random.default_rng(8)
    ops = {"pj": rng.normal(size=(n, h1)), "pi": rng.normal(size=(n, h1)), "edges": rng.normal(size=(e, fe)),
           "wc": rng.normal(size=(fe, h1)), "g": rng.normal(size=(n, h1))}
    g = {k: _t(v, F32).cuda() for k, v in ops.items()}
    cols = torch.from_numpy(np.stack([recv, send])).cuda().contiguous()
    ptr = torch.from_numpy(ptr0).cuda()
    ws, nbytes = _ffi.float_workspace("mp_inorp_edge_ws_bytes", e, h1, device=cols.device)
    head = [_ffi.ptr(g["pj"]), _ffi.ptr(g["pi"]), n, h1, _ffi.ptr(g["edges"]), fe, _ffi.ptr(g["wc"]), _ffi.ptr(cols), e,
            _ffi.ptr(ptr), None, _ffi.MP_ACT_TANH, 0.05, _ffi.MP_MEAN if method == "mean" else _ffi.MP_SUM]
    out = torch.full((n, h1), float("nan"), device="cuda")
    _ffi.call("mp_inorp_edge_f32", *head, _ffi.ptr(ws), nbytes, _ffi.ptr(out), _ffi.stream())
    gz = torch.full((e, h1), float("nan"), device="cuda")
    pi_bar = torch.full((n, h1), float("nan"), device="cuda")
    _ffi.call("mp_inorp_edge_grad_f32", *head, _ffi.ptr(g["g"]), _ffi.ptr(ws), nbytes, _ffi.ptr(gz), _ffi.ptr(pi_bar),
              _ffi.stream())
    keep = torch.from_numpy(valid)
    r, s = torch.from_numpy(recv[valid].astype(np.int64)), torch.from_numpy(send[valid].astype(np.int64))
    length = np.maximum(np.diff(ptr0), 1).astype(np.float64)       # the mean's divisor counts the skipped edges too
    refs = []
    for dt in (F32, F64):
        t = {k: _t(v, dt) for k, v in ops.items()}
        div = _t(length if method == "mean" else np.ones(n), dt)[:, None]
        want = ref.edge_kernel(t["pj"], t["pi"], t["edges"][keep], t["wc"], r, s, "tanh", "sum") / div
        rev = ref.edge_kernel_reverse(t["pj"], t["pi"], t["edges"][keep], t["wc"], r, s, "tanh", "sum", t["g"] / div)
        refs.append((want.numpy(), rev[0].numpy(), rev[1].numpy()))
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(gz).all()) and bool(torch.isfinite(pi_bar).all())
    for row in (2, 4, 5):                                          # no edges; only a skipped edge; no edges
        assert not out[row].any() and not pi_bar[row].any(), row
    assert_rows_close(out.cpu().numpy(), refs[0][0], refs[1][0], what="skipped edges %s: out" % method)
    assert not gz.cpu().numpy()[~valid].any()
    assert_rows_close(gz.cpu().numpy()[valid], refs[0][1], refs[1][1], what="skipped edges %s: gz" % method)
    assert_rows_close(pi_bar.cpu().numpy(), refs[0][2], refs[1][2], what="skipped edges %s: Pi_bar" % method)


def test_binary_reverse_of_a_one_row_operand():
    """``Binary``'s reverse sums a (1, W) operand's gradient over all rows (the step's ``c (N, 1) * b2 (1, W)`` and the
    sum behind it), for add, subtract and multiply, against torch's own broadcasting."""
    from gcnn_keras_amd.layers.modules import binary_values
    rng = np.random.default_rng(12)
    a_np, b_np, g_np = rng.normal(size=(37, 12)), rng.normal(size=(1, 12)), rng.normal(size=(37, 12))
    c_np = rng.normal(size=(37, 1))
    for op, fn in ((_ffi.MP_ADD, torch.add), (_ffi.MP_SUB, torch.sub), (_ffi.MP_MUL, torch.mul)):
        for left_np in (a_np, c_np):
            left = _t(left_np, F32).cuda().requires_grad_(True)
            row = _t(b_np, F32).cuda().requires_grad_(True)
            out = binary_values(op, left, row)
            gl, gr = torch.autograd.grad(out, [left, row], grad_outputs=_t(g_np, F32).cuda())
            refs = []
            for dt in (F32, F64):
                tl, tr = _t(left_np, dt).requires_grad_(True), _t(b_np, dt).requires_grad_(True)
                refs.append([x.numpy() for x in torch.autograd.grad(fn(tl, tr), [tl, tr], grad_outputs=_t(g_np, dt))])
            assert tuple(gr.shape) == (1, 12) and tuple(gl.shape) == tuple(left.shape)
            assert_rows_close(gr.cpu().numpy(), refs[0][1], refs[1][1], what="one-row operand, op %d" % op)
            assert_rows_close(gl.cpu().numpy(), refs[0][0], refs[1][0], what="left operand, op %d" % op)


# ----------------------------------------------------------------------------------------------------- the step
def make_step(node_width, edge_width, h1, h2, activation, method, use_bias=True, seed=0):
    lay = INorpEdgeStep(edge_mlp_args={"units": [h1, h2], "activation": [activation, "linear"], "use_bias": use_bias},
                        pooling_args={"pooling_method": method})
    lay.ensure_built([(None, None, node_width), (None, None, edge_width), (None, None, 2)])
    lay.use_fused_step = True       # off by default; these tests are about the fused route
    return lay


def step_case(kind, node_width, edge_width, h1, h2, activation, method, use_bias=True):
    b = ref.edge_list(kind)
    op = ref.step_operands(b, node_width, edge_width, h1, h2, use_bias=use_bias)
    lay = make_step(node_width, edge_width, h1, h2, activation, method, use_bias)
    arrays = [op["w1"], op["b1"], op["w2"], op["b2"]] if use_bias else [op["w1"], op["w2"]]
    lay.lay_mlp.set_weights(arrays)
    return b, op, lay


def step_inputs(b, op):
    ns, es = b["node_splits"], b["edge_splits"]
    return [_rag(op["nodes"], ns), _rag(op["edges"], es), _rag(b["edge_indices"], es)]


def restated_step(b, op, activation, method, dtype, coeff=None):
    """``(nu, [nodes_bar, edges_bar, W1_bar, b1_bar, W2_bar, b2_bar])`` of the reference's op sequence."""
    recv, send = ref.flat_indices(b)
    keys = [k for k in ("nodes", "edges", "w1", "b1", "w2", "b2") if op[k] is not None]
    t = {k: torch.tensor(op[k], dtype=dtype, requires_grad=True) for k in keys}
    layers = [(t["w1"], t.get("b1"), activation), (t["w2"], t.get("b2"), "linear")]
    nu = ref.round_tensor(t["nodes"], t["edges"], recv, send, layers, method)
    if coeff is None:
        return nu.detach().numpy(), None
    grads = torch.autograd.grad(nu, [t[k] for k in keys], grad_outputs=torch.as_tensor(coeff, dtype=dtype))
    return nu.detach().numpy(), [x.numpy() for x in grads]


@pytest.mark.parametrize("method", ["segment_sum", "segment_mean"])
@pytest.mark.parametrize("node_width", [3, 32, 41])
def test_step_on_both_routes(node_width, method):
    for k, kind in enumerate(ref.EDGE_LISTS):
        fe, h1 = EDGE_WIDTHS[k % 5], WIDTHS[k % 4]
        b, op, lay = step_case(kind, node_width, fe, h1, 20, "relu", method, use_bias=bool(k % 3))
        assert lay.fused_step
        x = step_inputs(b, op)
        with torch.no_grad():
            with engine_calls() as fused_names:
                fused = lay(x).values
            again = lay(x).values
            with engine_calls() as keyword_names:
                with_keyword = lay(x, training=False).values             # keyword arguments take the layer sequence
            lay.use_fused_step = False
            with engine_calls() as seq_names:
                seq = lay(x).values
        assert torch.equal(_bits(fused), _bits(again)) and torch.equal(_bits(seq), _bits(with_keyword))
        _fused_only(fused_names)
        _sequence_only(seq_names), _sequence_only(keyword_names)
        (r32, _), (r64, _) = (restated_step(b, op, "relu", method, dt) for dt in (F32, F64))
        what = "INorp step %s F=%d Fe=%d H1=%d %s" % (kind, node_width, fe, h1, method)
        assert_rows_close(fused.cpu().numpy(), r32, r64, what=what + ", fused")
        assert_rows_close(seq.cpu().numpy(), r32, r64, what=what + ", layer sequence")
        _twice_bar(fused.cpu().numpy(), seq.cpu().numpy(), r32, r64, what)
        recv, _ = ref.flat_indices(b)
        received = np.zeros(fused.shape[0], bool)
        received[recv.numpy()] = True
        assert not fused.cpu().numpy()[~received].any(), what + ": exactly 0 without edges"


@pytest.mark.parametrize("activation", ref.ACTIVATIONS)
def test_every_activation_against_the_layer_sequence(activation):
    b, op, lay = step_case("batch8", 7, 11, 64, 12, activation, "segment_mean")
    x = step_inputs(b, op)
    with torch.no_grad():
        fused = lay(x).values
        lay.use_fused_step = False
        seq = lay(x).values
    (r32, _), (r64, _) = (restated_step(b, op, activation, "segment_mean", dt) for dt in (F32, F64))
    assert_rows_close(fused.cpu().numpy(), r32, r64, what="INorp step %s, fused" % activation)
    assert_rows_close(seq.cpu().numpy(), r32, r64, what="INorp step %s, layer sequence" % activation)
    _twice_bar(fused.cpu().numpy(), seq.cpu().numpy(), r32, r64, "INorp step " + activation)


def taped_step(lay, b, op, coeff, fused):
    x = step_inputs(b, op)
    dense = lay.lay_mlp.mlp_dense_layer_list
    leaves = [x[0].values.requires_grad_(True), x[1].values.requires_grad_(True)]
    for d in dense:
        leaves += [t.requires_grad_(True) for t in (d.kernel, d.bias) if t is not None]
    lay.use_fused_step = fused
    try:
        with torch.enable_grad(), engine_calls() as calls:
            nu = lay(x).values
            grads = torch.autograd.grad(nu, leaves, grad_outputs=coeff)
    finally:
        lay.use_fused_step = True
        for t in leaves[2:]:
            t.requires_grad_(False)
    return nu.detach(), [t.detach() for t in grads], calls


@pytest.mark.parametrize("method", ["segment_sum", "segment_mean"])
@pytest.mark.parametrize("kind", ["e1", "e33", "e65", "star70", "cut1", "batch8", "batch8_shuffled"])
def test_step_on_a_tape(kind, method):
    """Every gradient of the step - nodes, edges (as embedded edge types need it), W1, b1, W2, b2 - from the fused rule,
    against autograd of the restatement and against the layer sequence's tape; equal bits on a second run."""
    k = ref.EDGE_LISTS.index(kind)
    fn, fe, h1, h2 = (3, 32, 41)[k % 3], EDGE_WIDTHS[k % 5], WIDTHS[k % 4], 12
    activation = "relu" if k % 2 else "swish"
    b, op, lay = step_case(kind, fn, fe, h1, h2, activation, method)
    n = int(b["node_splits"][-1])
    coeff = np.random.default_rng(9).normal(size=(n, h2)).astype(np.float32)
    cg = _t(coeff, F32).cuda()
    with torch.no_grad():
        plain = lay(step_inputs(b, op)).values
    nu, fused, fused_calls = taped_step(lay, b, op, cg, True)
    _, fused_again, _ = taped_step(lay, b, op, cg, True)
    nu_seq, seq, seq_calls = taped_step(lay, b, op, cg, False)
    assert torch.equal(_bits(nu), _bits(plain))                       # the tape runs the fused route's launches
    _fused_only(fused_calls, 1, 1)
    _sequence_only(seq_calls)
    print("[inorp] %s %s: engine calls of a taped step: fused %d, layer sequence %d" % (kind, method, len(fused_calls),
                                                                                     len(seq_calls)))
    for a, c in zip(fused, fused_again):
        assert torch.equal(_bits(a), _bits(c))
    (y32, g32), (y64, g64) = (restated_step(b, op, activation, method, dt, coeff) for dt in (F32, F64))
    what = "INorp step on a tape %s %s" % (kind, method)
    assert_rows_close(nu.cpu().numpy(), y32, y64, what=what + ": nu")
    for name, got, other, r32, r64 in zip(("nodes_bar", "edges_bar", "W1_bar", "b1_bar", "W2_bar", "b2_bar"), fused, seq,
                                          g32, g64):
        shape = _col if name == "edges_bar" else _vec
        if name == "edges_bar":
            _show_rowwise(what, got.cpu().numpy(), r32, r64)
        assert_rows_close(shape(got.cpu().numpy()), shape(r32), shape(r64), what="%s: %s" % (what, name))
        assert_rows_close(shape(other.cpu().numpy()), shape(r32), shape(r64), what="%s: %s, layer sequence" % (what, name))
        _twice_bar(shape(got.cpu().numpy()), shape(other.cpu().numpy()), shape(r32), shape(r64), "%s: %s" % (what, name))


def test_second_order_request_raises():
    """A backward through the first gradient (what a loss on that gradient does) reaches the fused rule's backward, which
    is first order.  ``backward()`` it is: ``once_differentiable`` hangs its error in front of leaves of its own, so a
    ``torch.autograd.grad`` towards a chosen tensor never runs it."""
    b, op, lay = step_case("e33", 5, 8, 32, 8, "swish", "segment_sum")
    x = step_inputs(b, op)
    x[0].values.requires_grad_(True)
    with engine_calls() as names:
        nu = lay(x).values
    _fused_only(names)
    g, = torch.autograd.grad(nu.sum(), x[0].values, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


def test_step_refuses_edges_out_of_range():
    b, op, lay = step_case("e33", 5, 8, 32, 8, "relu", "segment_sum")
    bad = b["edge_indices"].copy()
    bad[3, 1] = 25
    x = step_inputs(b, op)
    with pytest.raises(IndexError), torch.no_grad():
        lay([x[0], x[1], _rag(bad, b["edge_splits"])])


# ------------------------------------------------------------------------------------------------------ the model
def model_case(name, **extra):
    m = INorp.make_model(**dict(ref.CONFIGS[name], **extra))
    ws = ref.parity_weights(m, ref.WEIGHT_SEED[name])
    m.set_weights(ws)
    assert not m.use_fused_step     # off by default; the tests below switch the fused route on
    m.use_fused_step = True
    return m, ref.model_batch(synth, name), ws, ref.spec_of(INorp, name, **extra)


def model_inputs(b, cfg):
    ns, es = b["node_splits"], b["edge_splits"]
    spec = cfg["inputs"]
    nodes = _rag(b["node_attributes"], ns) if len(spec[0]["shape"]) >= 2 else _rag(b["node_number"].astype(np.float32), ns)
    edges = _rag(b["edge_attributes"], es) if len(spec[1]["shape"]) >= 2 else _rag(b["edge_number"].astype(np.float32), es)
    return [nodes, edges, _rag(b["edge_indices"], es), torch.from_numpy(b["graph_number"].astype(np.float32)).cuda()]


@pytest.mark.parametrize("name", ["esol", "mutag", "default"])
def test_model_eager_replayed_predict_and_switch(name):
    m, b, ws, cfg = model_case(name)
    served = 0 if name == "default" else 3
    assert m.fused_step_rounds == served
    x = model_inputs(b, cfg)
    r32, r64 = (ref.forward(ws, b, dt, cfg).numpy() for dt in (F32, F64))
    with torch.no_grad():
        with engine_calls() as fused_calls:
            eager = m(x)
        assert m.last_route == "eager"
        second, third = m(x), m(x)
        assert m.last_route == "graph"
        batched = m.predict(x, batch_size=5)
        m.use_fused_step = False
        assert not any(lay.use_fused_step for lay in m.step_layers)
        with engine_calls() as seq_calls:
            seq = m(x)
        assert m.last_route == "eager"                       # flipping the switch dropped the captured graphs
        m(x)
        seq_replayed = m(x)
        assert m.last_route == "graph"
        m.use_fused_step = True
        back = m(x)
        assert m.last_route == "eager"
    print("[inorp] %s: engine calls per forward: fused %d, layer sequence %d" % (name, len(fused_calls), len(seq_calls)))
    _sequence_only(seq_calls)
    if served:
        _fused_only(fused_calls, served)
    else:
        _sequence_only(fused_calls)                          # five layers 100 wide: the layer sequence either way
    assert torch.equal(eager, second) and torch.equal(eager, third) and torch.equal(eager, back)
    assert torch.equal(seq, seq_replayed)
    assert tuple(batched.shape) == (ref.GRAPHS, 1)
    what = "INorp " + name
    assert_rows_close(eager.cpu().numpy(), r32, r64, what=what + ", fused")
    assert_rows_close(seq.cpu().numpy(), r32, r64, what=what + ", layer sequence")
    assert_rows_close(batched.cpu().numpy(), r32, r64, what=what + ", predict(batch_size=5)")
    _twice_bar(eager.cpu().numpy(), seq.cpu().numpy(), r32, r64, what)


def test_model_node_output():
    m, b, ws, cfg = model_case("mutag", output_embedding="node")
    r32, r64 = (ref.forward(ws, b, dt, cfg).numpy() for dt in (F32, F64))
    with torch.no_grad():
        out = m(model_inputs(b, cfg))
    rows = out.values if isinstance(out, RaggedTensor) else out
    ns = b["node_splits"]
    assert tuple(rows.shape) == (ref.GRAPHS, int(np.max(np.diff(ns))), 1)   # output_to_tensor pads to the longest graph
    got = np.concatenate([rows[g, :ns[g + 1] - ns[g]].cpu().numpy() for g in range(ref.GRAPHS)])
    assert_rows_close(got, r32, r64, what="INorp node output")


@pytest.mark.parametrize("name", ["esol", "mutag", "default"])
def test_weight_gradients_of_every_weight(name):
    m, b, ws, cfg = model_case(name)
    x = model_inputs(b, cfg)
    target = ref.train_target(ref.GRAPHS)
    tg = torch.from_numpy(target).cuda()
    results = []
    m.requires_grad_(True)
    try:
        for fused in (True, False):
            m.use_fused_step = fused
            with torch.enable_grad(), engine_calls() as calls:
                loss = torch.abs(m(x) - tg).mean(dim=-1).mean()
                grads = torch.autograd.grad(loss, [t for _, t in m.weights])
            results.append((float(loss.detach()), grads, calls))
    finally:
        m.use_fused_step = True
        m.requires_grad_(False)
    (loss, grads, calls), (loss_seq, grads_seq, calls_seq) = results
    print("[inorp] %s: engine calls of a taped step: fused %d, layer sequence %d" % (name, len(calls), len(calls_seq)))
    _sequence_only(calls_seq)
    if m.fused_step_rounds:
        _fused_only(calls, 3, 3)                             # the tape took the fused rule in every block
    else:
        _sequence_only(calls)
    (l32, g32), (l64, g64) = (ref.weight_gradients(ws, b, dt, cfg, target) for dt in (F32, F64))
    np.testing.assert_allclose(loss, l64, rtol=1e-5)
    np.testing.assert_allclose(loss_seq, l64, rtol=1e-5)
    for (wname, _), got, other, r32, r64 in zip(m.weights, grads, grads_seq, g32, g64):
        assert float(np.abs(r64.numpy()).max()) > 0, wname
        assert_rows_close(_vec(got.cpu().numpy()), _vec(r32.numpy()), _vec(r64.numpy()),
                          what="INorp %s gradient of %s" % (name, wname))
        assert_rows_close(_vec(other.cpu().numpy()), _vec(r32.numpy()), _vec(r64.numpy()),
                          what="INorp %s gradient of %s, layer sequence" % (name, wname))


@pytest.mark.parametrize("name", ["esol", "mutag", "default"])
def test_three_training_steps(name):
    """Three SGD steps under the mean absolute error against the float64 restatement's steps: every loss at rtol 1e-5,
    every weight within 5e-5 of the tensor's largest total step plus two float32 ulps of the stored weight
    (tests/test_gpu_rgcn.py::test_one_training_step, per step); then the fused route serves the trained weights."""
    m, b, ws, cfg = model_case(name)
    x = model_inputs(b, cfg)
    target = ref.train_target(ref.GRAPHS)
    lr, steps = 0.005, 3      # small enough that no output crosses its target: the sign in the MAE gradient holds
    m.compile(optimizer=torch.optim.SGD(m.trainable_weights, lr=lr), loss="mean_absolute_error")
    losses = [m.train_on_batch(x, target) for _ in range(steps)]
    after = m.get_weights()
    assert not any(t.requires_grad for t in m.trainable_weights)
    want_losses, want = ref.sgd_steps(ws, b, cfg, target, lr, steps)
    np.testing.assert_allclose(losses, want_losses, rtol=1e-5)
    assert losses[2] < losses[0]
    for (wname, _), got, w0, w3 in zip(m.weights, after, ws, want):
        moved = float(np.max(np.abs(w3 - np.asarray(w0, np.float64))))
        assert moved > 0, wname
        assert np.max(np.abs(got - w3)) <= 5e-5 * moved + steps * 2.4e-7 * float(np.max(np.abs(w3))), wname
    with torch.no_grad(), engine_calls() as calls:
        out = m(x)
    assert calls.count("mp_inorp_edge_f32") == m.fused_step_rounds
    r32, r64 = (ref.forward(after, b, dt, cfg).numpy() for dt in (F32, F64))
    assert_rows_close(out.cpu().numpy(), r32, r64, what="INorp %s trained weights" % name)


def test_fit_under_binary_crossentropy():
    m, b, ws, cfg = model_case("mutag")                      # a sigmoid head
    x = model_inputs(b, cfg)
    target = (np.random.default_rng(6).uniform(size=(ref.GRAPHS, 1)) > 0.5).astype(np.float32)
    m.compile(optimizer=torch.optim.SGD(m.trainable_weights, lr=0.05), loss="binary_crossentropy")
    history = m.fit(x, target, batch_size=4, epochs=2, shuffle=False)
    assert len(history.history["loss"]) == 2 and all(np.isfinite(v) for v in history.history["loss"])
    assert any(not np.array_equal(a, c) for a, c in zip(ws, m.get_weights()))
    # one step on the whole batch: the loss is the restatement's binary cross-entropy
    m.set_weights(ws)
    prob = ref.forward(ws, b, F64, cfg).clamp(1e-7, 1 - 1e-7)
    t = torch.from_numpy(target).double()
    want = float(-(t * torch.log(prob + 1e-7) + (1 - t) * torch.log(1 - prob + 1e-7)).mean(dim=-1).mean())
    np.testing.assert_allclose(m.train_on_batch(x, target), want, rtol=1e-5)
    with torch.no_grad():
        out = m(x)
    after = m.get_weights()
    r32, r64 = (ref.forward(after, b, dt, cfg).numpy() for dt in (F32, F64))
    assert_rows_close(out.cpu().numpy(), r32, r64, what="INorp after fit, fused")


def test_set2set_infers_and_refuses_to_train():
    m, b, ws, cfg = model_case("mutag", use_set2set=True)
    x = model_inputs(b, cfg)
    with torch.no_grad():
        out = m(x)
        m.use_fused_step = False
        seq = m(x)
        m.use_fused_step = True
    assert tuple(out.shape) == (ref.GRAPHS, 1) and bool(torch.isfinite(out).all())
    assert_rows_close(out.cpu().numpy(), seq.cpu().numpy(), rtol=2e-5, what="INorp with Set2Set, fused vs layer sequence")
    before = m.get_weights()
    m.compile(optimizer="sgd", loss="mean_absolute_error")
    with pytest.raises(NotImplementedError, match="PoolingSet2Set|Set2Set"):
        m.train_on_batch(x, ref.train_target(ref.GRAPHS))
    assert all(np.array_equal(a, c) for a, c in zip(before, m.get_weights()))
    assert not any(t.requires_grad for t in m.trainable_weights)
