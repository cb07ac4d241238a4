"""Fused SchNet kernels (csrc/mp_cfconv.hip, csrc/mp_schnet_node.hip) through the C ABI vs the CPU oracle."""
import numpy as np
import pytest
import torch

from gcnn_keras_amd import synth
from oracle import kgcnn_oracle as ko
from parity import assert_rows_close, rowwise_rel

pytestmark = pytest.mark.gpu


def _rel_err(got, ref):
    """Per-ROW relative error (tests/parity.py): every node / graph row is held to the bar on its own magnitude."""
    return rowwise_rel(got, ref)


def _cfconv_case(seed, num_graphs=9, shuffle=False, bins=20):
    b = synth.qm9_like_batch(num_graphs=num_graphs, seed=seed)
    rng = np.random.default_rng(seed)
    idx = b["edge_indices"].copy()
    if shuffle:  # destroy the receiver order inside every graph
        for g in range(num_graphs):
            lo, hi = b["edge_splits"][g], b["edge_splits"][g + 1]
            idx[lo:hi] = idx[lo:hi][rng.permutation(hi - lo)]
    n = int(b["node_splits"][-1])
    x = ko.R(rng.normal(size=(n, 128)).astype(np.float32), b["node_splits"])
    xyz = ko.R(b["node_coordinates"], b["node_splits"])
    ridx = ko.R(idx, b["edge_splits"])
    p1, p2 = ko.node_position(xyz, ridx)
    dist = ko.node_distance_euclidean(p1, p2)
    rbf = ko.gauss_basis(dist, bins, 4.0, 0.4)
    p = {"dense1/kernel": synth.glorot_uniform(rng, bins, 128), "dense1/bias": rng.uniform(-.1, .1, 128).astype(np.float32),
         "dense2/kernel": synth.glorot_uniform(rng, 128, 128),
         "dense2/bias": rng.uniform(-.1, .1, 128).astype(np.float32)}
    return b, x, ridx, dist, rbf, p


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("variant", ["rbf", "gauss"])
@pytest.mark.parametrize("fast", [0, 1, 4, 5, 17])   # bit0: fast softplus, bit2: 8-wave workgroup, bit4: half the workgroups
def test_cfconv_fused_vs_oracle(shuffle, variant, fast):
    from gcnn_keras_amd import _ffi
    from gcnn_keras_amd.ragged import RaggedTensor
    b, x, ridx, dist, rbf, p = _cfconv_case(21, shuffle=shuffle)
    ref = ko.schnet_cfconv(x, rbf, ridx, p).values
    ref64 = ko.schnet_cfconv(ko.to_dtype(x, np.float64), ko.to_dtype(rbf, np.float64), ridx,
                             ko.to_dtype(p, np.float64)).values
    dx = RaggedTensor.from_numpy(x.values, x.row_splits)
    di = RaggedTensor.from_numpy(ridx.values, ridx.row_splits)
    plan = di.index_plan(dx)
    ptr, perm, seg = plan.csr(0)
    assert (perm is not None) == shuffle
    n, m = plan.N, plan.M
    out = torch.zeros((n, 128), dtype=torch.float32, device="cuda")
    w = {k: torch.from_numpy(v).cuda() for k, v in p.items()}
    send = plan.col(1).contiguous()
    packed = torch.empty(_ffi.lib().mp_cfconv_packed_floats(), dtype=torch.float32, device="cuda")
    _ffi.call("mp_cfconv_pack_f32", _ffi.ptr(w["dense1/kernel"]), _ffi.ptr(w["dense1/bias"]), 20,
              _ffi.ptr(w["dense2/kernel"]), _ffi.ptr(w["dense2/bias"]), _ffi.ptr(packed), _ffi.stream())
    if variant == "rbf":
        e = torch.from_numpy(rbf.values).cuda()
        _ffi.call("mp_cfconv_fused_f32", _ffi.ptr(dx.values), n, _ffi.ptr(e), 20, _ffi.ptr(packed),
                  _ffi.ptr(seg.contiguous()), _ffi.ptr(send), _ffi.ptr(perm), m, fast, _ffi.ptr(out), _ffi.stream())
    else:
        e = torch.from_numpy(dist.values.reshape(-1)).cuda()
        _ffi.call("mp_cfconv_gauss_fused_f32", _ffi.ptr(dx.values), n, _ffi.ptr(e), 20, 4.0, 0.4, 0.0,
                  _ffi.ptr(packed), _ffi.ptr(seg.contiguous()), _ffi.ptr(send), _ffi.ptr(perm), m, fast,
                  _ffi.ptr(out), _ffi.stream())
    got = out.cpu().numpy()
    assert _rel_err(got, ref) <= 1e-5                       # north_star tolerance for the float segment-sum
    assert _rel_err(got, ref64) <= max(4 * _rel_err(ref, ref64), 2e-6)


@pytest.mark.parametrize("flags", [0, 4])
@pytest.mark.parametrize("case", ["wide_range", "cancellation", "tiny"])
def test_cfconv_split_precision_gemm_keeps_the_fp32_error_budget(case, flags):
    """GEMM2 of the kernel runs on the bf16 matrix pipe as an FP32 emulation (three bf16 pieces per operand, six products,
    FP32 accumulate).  Inputs chosen against that scheme: second-layer weights spanning nine orders of magnitude in one
    column, columns that cancel to ~1e-4 of their terms, and weights near the bottom of the normal range.  The bar is
    the float32 NumPy oracle's own distance from its float64 twin (x4), i.e. the kernel may not be measurably worse than a
    k-ordered FP32 fma chain - plus the 1e-5 north-star bar against the float32 oracle."""
    from gcnn_keras_amd import _ffi
    from gcnn_keras_amd.ragged import RaggedTensor
    b, x, ridx, dist, rbf, p = _cfconv_case(33)
    rng = np.random.default_rng(5)
    p = {k: v.copy() for k, v in p.items()}
    w2 = p["dense2/kernel"]
    if case == "wide_range":
        w2 *= (10.0 ** rng.uniform(-6, 3, size=w2.shape)).astype(np.float32)
    elif case == "cancellation":      # rows pair up with opposite signs and nearly equal magnitude
        w2[1::2] = -w2[0::2] * (1.0 + 1e-4 * rng.standard_normal(w2[0::2].shape)).astype(np.float32)
        p["dense1/kernel"][:, 1::2] = p["dense1/kernel"][:, 0::2]
        p["dense1/bias"][1::2] = p["dense1/bias"][0::2]
    else:
        w2 *= np.float32(1e-30)
        p["dense2/bias"] *= np.float32(1e-30)
    ref = ko.schnet_cfconv(x, rbf, ridx, p).values
    ref64 = ko.schnet_cfconv(ko.to_dtype(x, np.float64), ko.to_dtype(rbf, np.float64), ridx,
                             ko.to_dtype(p, np.float64)).values
    dx = RaggedTensor.from_numpy(x.values, x.row_splits)
    di = RaggedTensor.from_numpy(ridx.values, ridx.row_splits)
    plan = di.index_plan(dx)
    _, perm, seg = plan.csr(0)
    out = torch.zeros((plan.N, 128), dtype=torch.float32, device="cuda")
    w = {k: torch.from_numpy(v).cuda() for k, v in p.items()}
    packed = torch.empty(_ffi.lib().mp_cfconv_packed_floats(), dtype=torch.float32, device="cuda")
    _ffi.call("mp_cfconv_pack_f32", _ffi.ptr(w["dense1/kernel"]), _ffi.ptr(w["dense1/bias"]), 20,
              _ffi.ptr(w["dense2/kernel"]), _ffi.ptr(w["dense2/bias"]), _ffi.ptr(packed), _ffi.stream())
    e = torch.from_numpy(rbf.values).cuda()
    _ffi.call("mp_cfconv_fused_f32", _ffi.ptr(dx.values), plan.N, _ffi.ptr(e), 20, _ffi.ptr(packed),
              _ffi.ptr(seg.contiguous()), _ffi.ptr(plan.col(1).contiguous()), _ffi.ptr(perm), plan.M, flags, _ffi.ptr(out),
              _ffi.stream())
    got = out.cpu().numpy()
    oracle_err = _rel_err(ref, ref64)
    assert _rel_err(got, ref64) <= max(4 * oracle_err, 2e-6), (case, _rel_err(got, ref64), oracle_err)
    assert _rel_err(got, ref) <= max(1e-5, 8 * oracle_err)


def _run_cfconv_gauss(x, ridx, dist, p, bins, flags):
    from gcnn_keras_amd import _ffi
    from gcnn_keras_amd.ragged import RaggedTensor
    dx = RaggedTensor.from_numpy(x.values, x.row_splits)
    di = RaggedTensor.from_numpy(ridx.values, ridx.row_splits)
    plan = di.index_plan(dx)
    _, perm, seg = plan.csr(0)
    out = torch.zeros((plan.N, 128), dtype=torch.float32, device="cuda")
    w = {k: torch.from_numpy(v).cuda() for k, v in p.items()}
    packed = torch.empty(_ffi.lib().mp_cfconv_packed_floats(), dtype=torch.float32, device="cuda")
    _ffi.call("mp_cfconv_pack_f32", _ffi.ptr(w["dense1/kernel"]), _ffi.ptr(w["dense1/bias"]), bins,
              _ffi.ptr(w["dense2/kernel"]), _ffi.ptr(w["dense2/bias"]), _ffi.ptr(packed), _ffi.stream())
    e = torch.from_numpy(dist.values.reshape(-1)).cuda()
    _ffi.call("mp_cfconv_gauss_fused_f32", _ffi.ptr(dx.values), plan.N, _ffi.ptr(e), bins, 4.0, 0.4, 0.0,
              _ffi.ptr(packed), _ffi.ptr(seg.contiguous()), _ffi.ptr(plan.col(1).contiguous()), _ffi.ptr(perm), plan.M, flags,
              _ffi.ptr(out), _ffi.stream())
    return out.cpu().numpy()


@pytest.mark.parametrize("flags", [0, 1, 5])
@pytest.mark.parametrize("bins", [20, 25, 7, 32])
def test_cfconv_basis_sizes_vs_oracle(bins, flags):
    """The basis sizes with their own builds - 20 (SchNet default) and 25 (the fork's force_schnet.py configuration): the
    first filter GEMM on the bf16 pipe, W1 pre-split into three bf16 pieces - and two sizes of the generic build (odd;
    the largest the kernel takes: FP32 matrix instructions for the first GEMM)."""
    b, x, ridx, dist, rbf, p = _cfconv_case(27, bins=bins)
    ref = ko.schnet_cfconv(x, rbf, ridx, p).values
    ref64 = ko.schnet_cfconv(ko.to_dtype(x, np.float64), ko.to_dtype(rbf, np.float64), ridx,
                             ko.to_dtype(p, np.float64)).values
    got = _run_cfconv_gauss(x, ridx, dist, p, bins, flags)
    assert _rel_err(got, ref) <= 1e-5
    assert _rel_err(got, ref64) <= max(4 * _rel_err(ref, ref64), 2e-6)


@pytest.mark.parametrize("bins", [20, 25])
@pytest.mark.parametrize("case", ["wide_range", "large_bias", "tiny"])
def test_cfconv_first_layer_split_precision(case, bins):
    """GEMM1 of the 20- and 25-bin builds is an FP32 emulation on the bf16 pipe as well (W1 | b1 and the basis values in
    three bf16 pieces, six products).  Inputs against that scheme: first-layer weights over nine orders of magnitude, a
    bias row that dominates the sum (the bias is one of the split rows), weights near the bottom of the normal range.
    Same bars as for GEMM2: the float32 oracle's own distance from its float64 twin."""
    b, x, ridx, dist, rbf, p = _cfconv_case(41, bins=bins)
    rng = np.random.default_rng(9)
    p = {k: v.copy() for k, v in p.items()}
    if case == "wide_range":
        p["dense1/kernel"] *= (10.0 ** rng.uniform(-6, 2, size=p["dense1/kernel"].shape)).astype(np.float32)
    elif case == "large_bias":
        p["dense1/bias"] = (rng.uniform(-1, 1, 128) * 37.0).astype(np.float32)
    else:
        p["dense1/kernel"] *= np.float32(1e-30)
        p["dense1/bias"] *= np.float32(1e-30)
    ref = ko.schnet_cfconv(x, rbf, ridx, p).values
    ref64 = ko.schnet_cfconv(ko.to_dtype(x, np.float64), ko.to_dtype(rbf, np.float64), ridx,
                             ko.to_dtype(p, np.float64)).values
    for flags in (0, 1):
        got = _run_cfconv_gauss(x, ridx, dist, p, bins, flags)
        oracle_err = _rel_err(ref, ref64)
        assert _rel_err(got, ref64) <= max(4 * oracle_err, 2e-6), (case, flags, _rel_err(got, ref64), oracle_err)
        assert _rel_err(got, ref) <= max(1e-5, 8 * oracle_err)


@pytest.mark.parametrize("flags", [1, 5, 17])
def test_cfconv_high_in_degree_segments_span_many_tiles(flags):
    """Receivers with more than 32 incoming edges: a segment then covers whole 32-edge tiles and is assembled from three
    or more float atomics (the order of which is not fixed) - still within the 1e-5 bar.  Also exercises a partial last
    tile, a receiver range that starts mid-tile and nodes without edges."""
    from gcnn_keras_amd import _ffi
    rng = np.random.default_rng(4)
    n = 40
    degrees = {0: 1, 3: 100, 4: 33, 9: 64, 17: 7, 39: 70}          # receiver -> in-degree; everything else isolated
    recv = np.concatenate([np.full(d, r) for r, d in sorted(degrees.items())])
    send = rng.integers(0, n, size=len(recv))
    idx = np.stack([recv, send], axis=1).astype(np.int64)
    m = len(idx)
    ns, es = np.array([0, n], dtype=np.int64), np.array([0, m], dtype=np.int64)
    x = ko.R(rng.normal(size=(n, 128)).astype(np.float32), ns)
    dist = ko.R(rng.uniform(0.5, 4.0, size=(m, 1)).astype(np.float32), es)
    rbf = ko.gauss_basis(dist, 20, 4.0, 0.4)
    p = {"dense1/kernel": synth.glorot_uniform(rng, 20, 128), "dense1/bias": rng.uniform(-.1, .1, 128).astype(np.float32),
         "dense2/kernel": synth.glorot_uniform(rng, 128, 128),
         "dense2/bias": rng.uniform(-.1, .1, 128).astype(np.float32)}
    ref = ko.schnet_cfconv(x, rbf, ko.R(idx, es), p).values
    w = {k: torch.from_numpy(v).cuda() for k, v in p.items()}
    packed = torch.empty(_ffi.lib().mp_cfconv_packed_floats(), dtype=torch.float32, device="cuda")
    _ffi.call("mp_cfconv_pack_f32", _ffi.ptr(w["dense1/kernel"]), _ffi.ptr(w["dense1/bias"]), 20,
              _ffi.ptr(w["dense2/kernel"]), _ffi.ptr(w["dense2/bias"]), _ffi.ptr(packed), _ffi.stream())
    out = torch.zeros((n, 128), dtype=torch.float32, device="cuda")
    dx, dd = torch.from_numpy(x.values).cuda(), torch.from_numpy(dist.values.reshape(-1)).cuda()
    dr, dsnd = torch.from_numpy(recv.astype(np.int32)).cuda(), torch.from_numpy(send.astype(np.int32)).cuda()
    _ffi.call("mp_cfconv_gauss_fused_f32", _ffi.ptr(dx), n, _ffi.ptr(dd), 20, 4.0, 0.4, 0.0, _ffi.ptr(packed),
              _ffi.ptr(dr), _ffi.ptr(dsnd), None, m, flags, _ffi.ptr(out), _ffi.stream())
    got = out.cpu().numpy()
    assert _rel_err(got, ref) <= 1e-5
    isolated = [r for r in range(n) if r not in degrees]
    assert np.all(got[isolated] == 0.0)                       # has_unconnected pad, kgcnn/layers/pooling.py:74-76


def _high_degree_case(seed=4):
    rng = np.random.default_rng(seed)
    n = 40
    degrees = {0: 1, 3: 100, 4: 33, 9: 64, 17: 7, 39: 70}          # receiver -> in-degree; everything else isolated
    recv = np.concatenate([np.full(d, r) for r, d in sorted(degrees.items())])
    send = rng.integers(0, n, size=len(recv))
    idx = np.stack([recv, send], axis=1).astype(np.int64)
    m = len(idx)
    ns, es = np.array([0, n], dtype=np.int64), np.array([0, m], dtype=np.int64)
    x = ko.R(rng.normal(size=(n, 128)).astype(np.float32), ns)
    dist = ko.R(rng.uniform(0.5, 4.0, size=(m, 1)).astype(np.float32), es)
    rbf = ko.gauss_basis(dist, 20, 4.0, 0.4)
    p = {"dense1/kernel": synth.glorot_uniform(rng, 20, 128), "dense1/bias": rng.uniform(-.1, .1, 128).astype(np.float32),
         "dense2/kernel": synth.glorot_uniform(rng, 128, 128),
         "dense2/bias": rng.uniform(-.1, .1, 128).astype(np.float32)}
    ref = ko.schnet_cfconv(x, rbf, ko.R(idx, es), p).values
    ref64 = ko.schnet_cfconv(ko.to_dtype(x, np.float64), ko.to_dtype(rbf, np.float64), ko.R(idx, es),
                             ko.to_dtype(p, np.float64)).values
    return n, m, recv, send, x, dist, p, ref, ref64


@pytest.mark.parametrize("flags", [33, 37, 49, 32])
def test_cfconv_deterministic_mode_is_bit_reproducible(flags):
    """flags bit 5: boundary partials are parked in a workspace and added per receiver in edge order by a second kernel
    (no float atomics).  Receivers with 33..100 incoming edges span several 32-edge tiles - the case where the default mode
    may differ in the last bit between runs; here repeated launches must agree bit for bit, and every row holds the 1e-5 bar."""
    import ctypes
    from gcnn_keras_amd import _ffi
    n, m, recv, send, x, dist, p, ref, ref64 = _high_degree_case()
    w = {k: torch.from_numpy(v).cuda() for k, v in p.items()}
    packed = torch.empty(_ffi.lib().mp_cfconv_packed_floats(), dtype=torch.float32, device="cuda")
    _ffi.call("mp_cfconv_pack_f32", _ffi.ptr(w["dense1/kernel"]), _ffi.ptr(w["dense1/bias"]), 20,
              _ffi.ptr(w["dense2/kernel"]), _ffi.ptr(w["dense2/bias"]), _ffi.ptr(packed), _ffi.stream())
    nbytes = ctypes.c_size_t(0)
    _ffi.call("mp_cfconv_det_workspace_bytes", m, ctypes.byref(nbytes))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
    dx, dd = torch.from_numpy(x.values).cuda(), torch.from_numpy(dist.values.reshape(-1)).cuda()
    dr, dsnd = torch.from_numpy(recv.astype(np.int32)).cuda(), torch.from_numpy(send.astype(np.int32)).cuda()
    outs = []
    for _ in range(4):
        out = torch.zeros((n, 128), dtype=torch.float32, device="cuda")
        _ffi.call("mp_cfconv_gauss_fused_ws_f32", _ffi.ptr(dx), n, _ffi.ptr(dd), 20, 4.0, 0.4, 0.0, _ffi.ptr(packed),
                  _ffi.ptr(dr), _ffi.ptr(dsnd), None, m, flags, _ffi.ptr(out), _ffi.ptr(ws), nbytes.value, _ffi.stream())
        outs.append(out.clone())
    torch.cuda.synchronize()
    assert all(torch.equal(outs[0], o) for o in outs[1:])
    assert_rows_close(outs[0].cpu().numpy(), ref, ref64, what="deterministic cfconv")
    # without the workspace the flag is refused rather than silently ignored
    assert _ffi.lib().mp_cfconv_gauss_fused_ws_f32(_ffi.ptr(dx), n, _ffi.ptr(dd), 20, 4.0, 0.4, 0.0, _ffi.ptr(packed),
                                                   _ffi.ptr(dr), _ffi.ptr(dsnd), None, m, flags,
                                                   _ffi.ptr(outs[0]), None, 0, _ffi.stream()) == _ffi.MP_EINVAL


def test_cfconv_deterministic_mode_on_a_real_batch_matches_default_mode():
    """On a QM9-shaped batch (in-degree <= 30) both modes must give the same bits: there every boundary receiver gets at
    most two partials, and a + b == b + a."""
    import ctypes
    from gcnn_keras_amd import _ffi
    from gcnn_keras_amd.ragged import RaggedTensor
    b, x, ridx, dist, rbf, p = _cfconv_case(5, num_graphs=40)
    dx = RaggedTensor.from_numpy(x.values, x.row_splits)
    di = RaggedTensor.from_numpy(ridx.values, ridx.row_splits)
    plan = di.index_plan(dx)
    _, perm, seg = plan.csr(0)
    assert perm is None
    n, m = plan.N, plan.M
    w = {k: torch.from_numpy(v).cuda() for k, v in p.items()}
    packed = torch.empty(_ffi.lib().mp_cfconv_packed_floats(), dtype=torch.float32, device="cuda")
    _ffi.call("mp_cfconv_pack_f32", _ffi.ptr(w["dense1/kernel"]), _ffi.ptr(w["dense1/bias"]), 20,
              _ffi.ptr(w["dense2/kernel"]), _ffi.ptr(w["dense2/bias"]), _ffi.ptr(packed), _ffi.stream())
    nbytes = ctypes.c_size_t(0)
    _ffi.call("mp_cfconv_det_workspace_bytes", m, ctypes.byref(nbytes))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
    e = torch.from_numpy(dist.values.reshape(-1)).cuda()
    outs = {}
    for flags in (1, 33):
        out = torch.zeros((n, 128), dtype=torch.float32, device="cuda")
        _ffi.call("mp_cfconv_gauss_fused_ws_f32", _ffi.ptr(dx.values), n, _ffi.ptr(e), 20, 4.0, 0.4, 0.0,
                  _ffi.ptr(packed), _ffi.ptr(seg.contiguous()), _ffi.ptr(plan.col(1).contiguous()), None, m, flags,
                  _ffi.ptr(out), _ffi.ptr(ws), nbytes.value, _ffi.stream())
        outs[flags] = out
    torch.cuda.synchronize()
    assert torch.equal(outs[1], outs[33])
    assert_rows_close(outs[33].cpu().numpy(), ko.schnet_cfconv(x, rbf, ridx, p).values, what="det cfconv, QM9 batch")


def test_cfconv_refuses_a_basis_wider_than_32_and_accepts_an_empty_problem():
    from gcnn_keras_amd import _ffi
    lib = _ffi.lib()
    assert lib.mp_cfconv_fused_f32(None, 4, None, 40, None, None, None, None, 3, 0, None,
                                   None) == _ffi.MP_EINVAL      # basis too wide for the fused kernel
    assert lib.mp_cfconv_fused_f32(None, 0, None, 20, None, None, None, None, 0, 0, None,
                                   None) == _ffi.MP_OK           # empty problem


@pytest.mark.parametrize("num_graphs,seed,shuffle", [(6, 11, False), (1, 5, False), (128, 1234, False),
                                                     (17, 3, True)])
def test_fused_schnet_forward(num_graphs, seed, shuffle):
    from gcnn_keras_amd.engine import SchnetForward
    b = synth.qm9_like_batch(num_graphs=num_graphs, seed=seed)
    if shuffle:
        rng = np.random.default_rng(0)
        idx = b["edge_indices"].copy()
        for g in range(num_graphs):
            lo, hi = b["edge_splits"][g], b["edge_splits"][g + 1]
            idx[lo:hi] = idx[lo:hi][rng.permutation(hi - lo)]
        b["edge_indices"] = idx
    p = synth.schnet_params(seed=7, random_bias=True)
    fwd = SchnetForward(p, depth=3, mode="fused")
    assert fwd.mode == "fused"
    fwd.load_batch(b)
    out1 = fwd.forward().cpu().numpy().copy()
    out2 = fwd.forward().cpu().numpy().copy()      # graph replay: same result, aggregation buffer was re-zeroed
    fwd.check_flags()
    assert np.array_equal(out1, out2)
    ref = ko.schnet_forward(p, ko.R(b["node_number"], b["node_splits"]), ko.R(b["node_coordinates"], b["node_splits"]),
                            ko.R(b["edge_indices"], b["edge_splits"]), depth=3)
    ref64 = ko.schnet_forward(ko.to_dtype(p, np.float64), ko.R(b["node_number"], b["node_splits"]),
                              ko.R(b["node_coordinates"].astype(np.float64), b["node_splits"]),
                              ko.R(b["edge_indices"], b["edge_splits"]), depth=3)
    assert out1.shape == ref.shape
    assert _rel_err(out1, ref) <= 1e-5
    assert _rel_err(out1, ref64) <= max(4 * _rel_err(ref, ref64), 2e-6)
    # the layer-by-layer path gives the same answer within the same budget
    lay = SchnetForward(p, depth=3, mode="layers")
    lay.load_batch(b)
    assert _rel_err(lay.forward().cpu().numpy(), out1) <= 1e-5


@pytest.mark.parametrize("case", ["wide_range", "cancellation"])
def test_node_kernels_on_the_bf16_pipe_keep_the_fp32_error_budget(case, monkeypatch):
    """The forward's node kernels run their GEMMs on the bf16 matrix pipe as an FP32 emulation (three bf16 pieces per
    operand, six products: csrc/mp_node_tile.h).  Node-side weights chosen against the scheme - magnitudes over six orders,
    rows that cancel - must leave the forward as close to the float64 twin as the FP32 matrix instructions do
    (MPENGINE_NODE_BF16=0) and inside the float32 oracle's own distance from it."""
    from gcnn_keras_amd.engine import SchnetForward
    b = synth.qm9_like_batch(num_graphs=9, seed=17)
    p = {k: (None if v is None else v.copy()) for k, v in synth.schnet_params(seed=11, random_bias=True).items()}
    rng = np.random.default_rng(3)
    for i in range(3):
        for name in ("interaction%d/dense2/kernel" % i, "interaction%d/dense3/kernel" % i):
            w = p[name]
            if case == "wide_range":
                w *= (10.0 ** rng.uniform(-4, 2, size=w.shape)).astype(np.float32) * np.float32(0.05)
            else:
                w[1::2] = -w[0::2] * (1.0 + 1e-4 * rng.standard_normal(w[0::2].shape)).astype(np.float32)
    args = (ko.R(b["node_number"], b["node_splits"]), ko.R(b["node_coordinates"], b["node_splits"]),
            ko.R(b["edge_indices"], b["edge_splits"]))
    ref = ko.schnet_forward(p, *args, depth=3)
    ref64 = ko.schnet_forward(ko.to_dtype(p, np.float64), args[0], ko.R(b["node_coordinates"].astype(np.float64),
                                                                       b["node_splits"]), args[2], depth=3)
    oracle_err = _rel_err(ref, ref64)
    errs = {}
    for bf in ("1", "0"):
        monkeypatch.setenv("MPENGINE_NODE_BF16", bf)
        fwd = SchnetForward(p, depth=3, mode="fused")
        fwd.load_batch(b)
        out = fwd.forward().cpu().numpy().copy()
        fwd.check_flags()
        errs[bf] = _rel_err(out, ref64)
        assert errs[bf] <= max(4 * oracle_err, 2e-6), (case, bf, errs[bf], oracle_err)
        assert _rel_err(out, ref) <= max(1e-5, 8 * oracle_err)
    assert errs["1"] <= max(2 * errs["0"], 2e-6), errs


def test_fused_schnet_empty_graphs_and_isolated_nodes():
    from gcnn_keras_amd.engine import SchnetForward
    b = synth.qm9_like_batch(num_graphs=5, seed=2)
    # append a graph with 3 nodes and no edges, then an empty graph (dropped by PoolingNodes like TF does)
    b["node_number"] = np.concatenate([b["node_number"], np.array([6., 1., 8.], np.float32)])
    b["node_coordinates"] = np.concatenate([b["node_coordinates"], np.zeros((3, 3), np.float32)])
    n, m = b["node_splits"][-1], b["edge_splits"][-1]
    b["node_splits"] = np.concatenate([b["node_splits"], [n + 3, n + 3]])
    b["edge_splits"] = np.concatenate([b["edge_splits"], [m, m]])
    p = synth.schnet_params(seed=7, random_bias=True)
    fwd = SchnetForward(p, depth=3, mode="fused")
    fwd.load_batch(b)
    out = fwd.forward().cpu().numpy()
    ref = ko.schnet_forward(p, ko.R(b["node_number"], b["node_splits"]), ko.R(b["node_coordinates"], b["node_splits"]),
                            ko.R(b["edge_indices"], b["edge_splits"]), depth=3)
    assert out.shape == ref.shape == (6, 1)
    assert _rel_err(out, ref) <= 1e-5


def test_forwards_in_flight_are_independent_and_identical():
    """``SchnetForward(in_flight=k)``: k batch slots (own buffers / stream / graph, 256-register cfconv build) replayed
    concurrently give, each, the bits of a lone forward of the same build and stay within 1e-5 of the oracle."""
    from gcnn_keras_amd.engine import SchnetForward
    b = synth.qm9_like_batch(num_graphs=128, seed=1234)
    p = synth.schnet_params(seed=7, random_bias=True)
    multi = SchnetForward(p, depth=3, mode="fused", in_flight=3)
    multi.load_batch(b)
    last = {}
    for i in range(30):                      # slots overlap on the GPU
        last[i % 3] = multi.replay(i)
    torch.cuda.synchronize()
    outs = [last[k].clone() for k in range(3)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    lone = multi.forward(0).clone()
    torch.cuda.synchronize()
    assert torch.equal(lone, outs[0])
    ref = ko.schnet_forward(p, ko.R(b["node_number"], b["node_splits"]), ko.R(b["node_coordinates"], b["node_splits"]),
                            ko.R(b["edge_indices"], b["edge_splits"]), depth=3)
    got = outs[0].cpu().numpy()
    assert_rows_close(got, ref, what="forwards in flight")
    multi.check_flags()


def test_direct_forward_launch_equals_graph_replay():
    """``mp_schnet_forward_launch`` (one C-ABI call, no capture) issues the same eight launches as the captured graph."""
    from gcnn_keras_amd.engine import SchnetForward
    b = synth.qm9_like_batch(num_graphs=17, seed=33)
    p = synth.schnet_params(seed=7, random_bias=True)
    fwd = SchnetForward(p, depth=3, mode="fused", in_flight=1)
    fwd.load_batch(b)
    slot = fwd._slots[0]
    replayed = slot.replay().clone()
    torch.cuda.synchronize()
    slot.out.zero_()
    with torch.cuda.stream(slot.stream):
        direct = slot.launch_direct().clone()
    torch.cuda.synchronize()
    assert torch.equal(direct, replayed)
    ref = ko.schnet_forward(p, ko.R(b["node_number"], b["node_splits"]), ko.R(b["node_coordinates"], b["node_splits"]),
                            ko.R(b["edge_indices"], b["edge_splits"]), depth=3)
    assert_rows_close(direct.cpu().numpy(), ref, what="direct forward launch")
    slot.check_flags()


def test_slots_with_unsorted_receivers_and_direct_launch_fallback():
    """Batches whose receivers are not sorted take the stable-sort route inside every slot; ``launch_direct`` (built for
    sorted batches) must fall back to the graph replay and still return the same bits."""
    from gcnn_keras_amd.engine import SchnetForward
    b = synth.qm9_like_batch(num_graphs=11, seed=8)
    rng = np.random.default_rng(1)
    idx = b["edge_indices"].copy()
    for g in range(11):
        lo, hi = b["edge_splits"][g], b["edge_splits"][g + 1]
        idx[lo:hi] = idx[lo:hi][rng.permutation(hi - lo)]
    b["edge_indices"] = idx
    p = synth.schnet_params(seed=7, random_bias=True)
    fwd = SchnetForward(p, depth=3, mode="fused", in_flight=2)
    fwd.load_batch(b)
    assert not fwd._slots[0].sorted
    last = {}
    for i in range(6):
        last[i % 2] = fwd.replay(i)
    torch.cuda.synchronize()
    a, c = last[0].clone(), last[1].clone()
    assert torch.equal(a, c)
    with torch.cuda.stream(fwd._slots[0].stream):
        d = fwd._slots[0].launch_direct().clone()
    torch.cuda.synchronize()
    assert torch.equal(d, a)
    ref = ko.schnet_forward(p, ko.R(b["node_number"], b["node_splits"]), ko.R(b["node_coordinates"], b["node_splits"]),
                            ko.R(b["edge_indices"], b["edge_splits"]), depth=3)
    assert _rel_err(a.cpu().numpy(), ref) <= 1e-5
    fwd.check_flags()


def test_model_call_returns_a_tensor_nobody_else_holds():
    """``model(inputs)`` on a re-bound batch replays a graph whose readout writes into one of the slot's result buffers
    (no copy launch); a buffer is handed out only while no caller holds it or a view of it, so results behave like the
    fresh tensors a Keras call returns: held results are never written again, dropped ones are recycled."""
    from gcnn_keras_amd import _ffi
    from gcnn_keras_amd.literature import Schnet
    from gcnn_keras_amd.ragged import RaggedTensor
    b = synth.qm9_like_batch(num_graphs=9, seed=5)
    p = synth.schnet_params(seed=7, random_bias=True)
    model = Schnet.make_model(depth=3)
    model.set_weights(list(p.values()))
    xyz = RaggedTensor.from_numpy(b["node_coordinates"], b["node_splits"])
    inputs = [RaggedTensor.from_numpy(b["node_number"], b["node_splits"]), xyz,
              RaggedTensor.from_numpy(b["edge_indices"], b["edge_splits"])]
    first = model(inputs)                       # bind + direct launch (copy of the static buffer)
    held = [model(inputs) for _ in range(5)]    # more results held than the ring has buffers
    torch.cuda.synchronize()
    ptrs = {t.data_ptr() for t in held} | {first.data_ptr()}
    assert len(ptrs) == 6                       # all distinct storages
    want = first.clone()
    assert all(torch.equal(t, want) for t in held)
    view = held[0][:3]                          # a view keeps its buffer out of circulation too
    base_ptr = held[0].data_ptr()
    del held
    xyz.values.mul_(1.05)                       # new coordinates in the bound tensor: later calls give other numbers
    later = [model(inputs) for _ in range(4)]
    torch.cuda.synchronize()
    assert all(t.data_ptr() != base_ptr for t in later)
    assert torch.equal(view, want[:3]) and torch.equal(first, want)
    assert not torch.equal(later[0], want) and all(torch.equal(t, later[0]) for t in later)
    ref = ko.schnet_forward(p, ko.R(b["node_number"], b["node_splits"]),
                            ko.R(b["node_coordinates"] * np.float32(1.05), b["node_splits"]),
                            ko.R(b["edge_indices"], b["edge_splits"]), depth=3)
    assert _rel_err(later[0].cpu().numpy(), ref) <= 1e-5
    # a loop that drops its results runs on the ring alone: one graph launch per call, the buffers come round again
    del later, view
    before = _ffi.launch_count()
    seen = {model(inputs).data_ptr() for _ in range(8)}
    assert _ffi.launch_count() - before == 8 and len(seen) <= 3
    assert model.fused.last == "graph"


def test_launch_group_serves_several_batches_from_one_launch_sequence():
    """``route.call_group([inputs_a, inputs_b, ...])``: the members concatenated on the device (``mp_concat_batches``) and
    run as one union batch - every member gets the rows of a forward of its own (graphs do not interact; the cfconv
    boundary sums pair differently: 2e-6), against the oracle too; replayed from the group's graph on the second call,
    following in-place coordinate updates of a member; a member that ends in a graph without nodes keeps its own row count."""
    from gcnn_keras_amd.literature import Schnet
    from helpers import dev
    p = synth.schnet_params(seed=7, random_bias=True)
    model = Schnet.make_model(depth=3)
    model.set_weights(list(p.values()))
    batches = [synth.qm9_like_batch(num_graphs=g, seed=s) for g, s in ((5, 1), (9, 2), (1, 3), (7, 4))]
    b3 = batches[3]                                      # a trailing graph without nodes (and edges) in the last member ...
    b3["node_splits"] = np.concatenate([b3["node_splits"], b3["node_splits"][-1:]])
    b3["edge_splits"] = np.concatenate([b3["edge_splits"], b3["edge_splits"][-1:]])
    b1 = batches[1]                                      # ... and in a middle one
    b1["node_splits"] = np.concatenate([b1["node_splits"], b1["node_splits"][-1:]])
    b1["edge_splits"] = np.concatenate([b1["edge_splits"], b1["edge_splits"][-1:]])
    ins = [[dev(b["node_number"], b["node_splits"]), dev(b["node_coordinates"], b["node_splits"]),
            dev(b["edge_indices"], b["edge_splits"])] for b in batches]

    def oracle(b):
        return ko.schnet_forward(p, ko.R(b["node_number"], b["node_splits"]), ko.R(b["node_coordinates"], b["node_splits"]),
                                 ko.R(b["edge_indices"], b["edge_splits"]), depth=3)

    alone = [model(x).cpu().numpy() for x in ins]
    got = model.fused.call_group(ins)
    assert model.fused.last == "direct" and len(got) == 4
    again = model.fused.call_group(ins)
    assert model.fused.last == "graph"
    for k, b in enumerate(batches):
        g_own = len(b["node_splits"]) - 1 - (1 if k in (1, 3) else 0)       # the member's own trailing empty graph dropped
        assert tuple(got[k].shape) == (g_own, 1) == alone[k].shape
        assert torch.equal(got[k], again[k])
        assert rowwise_rel(got[k].cpu().numpy(), alone[k]) <= 2e-6
        assert_rows_close(got[k].cpu().numpy(), oracle(b), what="launch group, member %d" % k)
    # results are fresh tensors: a held result is not overwritten by the next call
    keep = [t.clone() for t in again]
    ins[2][1].values.mul_(1.01)                          # new coordinates for member 2 only
    third = model.fused.call_group(ins)
    for k in range(4):
        assert torch.equal(again[k], keep[k])
        assert torch.equal(third[k], keep[k]) == (k != 2)
    batches[2]["node_coordinates"] = batches[2]["node_coordinates"] * np.float32(1.01)
    assert_rows_close(third[2].cpu().numpy(), oracle(batches[2]), what="launch group, updated member")
    model.fused.check_flags()


def test_first_sight_groups_recycle_their_work_set_and_union_tensors():
    """Never-seen batches served as launch groups (``model.predict`` over a dataset, five batches per launch sequence): the
    union's input tensors and the concatenation descriptor live in the work set, a dropped group hands its set back at once
    (no reference cycle between group and slot), the next group of the same size class takes it - nothing allocated - and
    gets the oracle's rows, not the previous group's; the first result is the slot's own buffer (no copy launch)."""
    import gc
    from gcnn_keras_amd.data.packer import BatchPacker
    from gcnn_keras_amd.literature import Schnet
    p = synth.schnet_params(seed=7, random_bias=True)
    model = Schnet.make_model(depth=3)
    model.set_weights(list(p.values()))
    items = [{"name": "node_number", "ragged": True, "dtype": "float32"},
             {"name": "node_coordinates", "ragged": True, "dtype": "float32"},
             {"name": "edge_indices", "ragged": True, "dtype": "int64"}]
    packer = BatchPacker(items, index_item="edge_indices", node_item="node_number", slots=8)

    def graph_list(b):
        ns, es = b["node_splits"], b["edge_splits"]
        return [{"node_number": b["node_number"][ns[g]:ns[g + 1]], "node_coordinates": b["node_coordinates"][ns[g]:ns[g + 1]],
                 "edge_indices": b["edge_indices"][es[g]:es[g + 1]]} for g in range(len(ns) - 1)]

    def oracle(b):
        return ko.schnet_forward(p, ko.R(b["node_number"], b["node_splits"]), ko.R(b["node_coordinates"], b["node_splits"]),
                                 ko.R(b["edge_indices"], b["edge_splits"]), depth=3)

    gc.disable()                                     # a cycle would be hidden by a collection that happens to run
    try:
        route = model.fused
        made = []
        for rnd in range(3):
            batches = [synth.qm9_like_batch(num_graphs=12, seed=100 + 4 * rnd + k) for k in range(4)]
            packed = [packer.pack(graph_list(b)) for b in batches]
            for pb in packed:
                pb.wait(torch.cuda.current_stream())
            ins = [[pb["node_number"], pb["node_coordinates"], pb["edge_indices"]] for pb in packed]
            got = route.call_group(ins)
            assert route.last == "direct"
            torch.cuda.synchronize()
            for k, b in enumerate(batches):
                assert_rows_close(got[k].cpu().numpy(), oracle(b), what="first-sight group %d, member %d" % (rnd, k))
            grp = next(iter(route._groups.values()))
            assert got[0].untyped_storage().data_ptr() == grp.slot.out.untyped_storage().data_ptr()   # handed out, not copied
            del grp
            route._groups.clear()                    # the group is dropped: its work set must be back in the arena NOW
            made.append(route._arena.made)
            assert sum(len(v) for v in route._arena.free.values()) >= 1
            del got, ins, packed
        assert made[0] == made[1] == made[2], made   # rounds 2 and 3 took round 1's set (same size class)
        assert route._arena.taken >= 2
    finally:
        gc.enable()
    route.check_flags()


def test_schnet_forward_harness_launch_groups_in_flight():
    """``SchnetForward(group=k, in_flight=n)`` (what ``bench.py`` times by default): n launch groups of k independent batches
    each; every member's rows equal a lone forward's (2e-6: the cfconv boundary sums pair differently in the union), the
    groups overlap on their streams and return the same bits replay after replay."""
    from gcnn_keras_amd.engine import SchnetForward
    b = synth.qm9_like_batch(num_graphs=24, seed=5)
    p = synth.schnet_params(seed=7, random_bias=True)
    fwd = SchnetForward(p, depth=3, mode="fused", in_flight=2, group=3)
    fwd.load_batch(b)
    lone = fwd.forward(0).clone()
    first = {}
    for j in range(6):
        outs = fwd.replay_group(j)
        assert len(outs) == 3
        if j < 2:
            first[j] = [o.clone() for o in outs]
    torch.cuda.set_stream(torch.cuda.default_stream())
    torch.cuda.synchronize()
    for j in range(2):
        again = fwd.replay_group(j)
        torch.cuda.synchronize()
        for o, f in zip(again, first[j]):
            assert torch.equal(o, f) and tuple(o.shape) == (24, 1)
            assert rowwise_rel(o.cpu().numpy(), lone.cpu().numpy()) <= 2e-6
    torch.cuda.set_stream(torch.cuda.default_stream())
    ref = ko.schnet_forward(p, ko.R(b["node_number"], b["node_splits"]), ko.R(b["node_coordinates"], b["node_splits"]),
                            ko.R(b["edge_indices"], b["edge_splits"]), depth=3)
    assert_rows_close(first[0][1].cpu().numpy(), ref, what="launch group member through the harness")
    fwd.check_flags()
