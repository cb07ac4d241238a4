"""Figures behind the cfconv filter table, measured on the GPU:

1. the MFMA kernel's own error against float64 on the self-check distances of the table build - one edge per receiver,
   x all ones, so out[e] is the filter row of edge e - and the table's error on the same distances: the bar
   ``fused.FILTER_TABLE_BAR`` is twice the first figure;
2. the duration of one weight update's table builds (three blocks, build + self-check + read-back);
3. the table kernel at 4, 8 and 16 waves per workgroup and the MFMA kernel on a union-sized (4093 tiles) and a lone
   (819 tiles) edge list.

    python scripts/probe_filter_table.py
"""
import ctypes
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gcnn_keras_amd import _ffi, fused, synth  # noqa: E402

F = 128
GAUSS = {"bins": 20, "distance": 4.0, "offset": 0.0, "sigma": 0.4}
f32 = np.float32


def filter64(v, w1, b1, w2, b2):
    mu = np.arange(GAUSS["bins"], dtype=np.float64) / GAUSS["bins"] * float(f32(GAUSS["distance"]))
    gamma = 1.0 / float(f32(GAUSS["sigma"])) ** 2 / 2.0
    g = np.exp(-gamma * (np.asarray(v, np.float64)[:, None] - mu) ** 2)
    hid = np.logaddexp(0.0, g @ w1.astype(np.float64) + b1.astype(np.float64)) - np.log(2.0)
    return hid @ w2.astype(np.float64) + b2.astype(np.float64)


def check_distances(lay):
    h = f32(1.0 / lay.inv_h)
    q = np.arange(3 * lay.n_int)
    v = (f32(lay.v_lo) + ((q // 3).astype(f32) + f32(0.25) * (q % 3 + 1).astype(f32)) * h).astype(f32)
    ends = np.array([max(lay.v_lo - 1.0, -GAUSS["offset"]), lay.v_end + 0.015625, lay.v_end + 4.0, lay.v_end + 1000.0], f32)
    return (np.concatenate([v, ends]) + f32(GAUSS["offset"])).astype(f32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def timed(fn, iters=30):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def main():
    p = {k: v for k, v in synth.schnet_params(seed=7, random_bias=True).items()}
    pd = {k: dev(np.asarray(v, np.float32)) for k, v in p.items() if v is not None}
    lay = fused.filter_table_layout(GAUSS)
    d = check_distances(lay)
    m = len(d)
    x = torch.ones((m, F), dtype=torch.float32, device="cuda")
    recv = torch.arange(m, dtype=torch.int32, device="cuda")
    send = torch.zeros(m, dtype=torch.int32, device="cuda")
    dist = dev(d)
    images = fused.pack_weights(pd, 3, GAUSS["bins"], gauss=GAUSS)
    ft = images["ftable"]
    print("layout: v_lo %g v_end %g 1/h %g intervals %d rows %d (%.1f KB)" % (
        lay.v_lo, lay.v_end, lay.inv_h, lay.n_int, lay.rows, lay.rows * 0.5))
    for i in range(3):
        pre = "interaction%d/cfconv/" % i
        w = [p[pre + k] for k in ("dense1/kernel", "dense1/bias", "dense2/kernel", "dense2/bias")]
        ref = filter64((d - f32(GAUSS["offset"])).astype(f32), *w)
        scale = float(np.max(np.abs(ref)))
        res = {}
        for name in ("mfma", "table"):
            out = torch.zeros((m, F), dtype=torch.float32, device="cuda")
            if name == "mfma":
                _ffi.call("mp_cfconv_gauss_fused_f32", _ffi.ptr(x), m, _ffi.ptr(dist), GAUSS["bins"], GAUSS["distance"],
                          GAUSS["sigma"], GAUSS["offset"], _ffi.ptr(images["cfconv"][i]), _ffi.ptr(recv), _ffi.ptr(send),
                          None, m, 1, _ffi.ptr(out), _ffi.stream())
            else:
                _ffi.call("mp_cfconv_table_f32", _ffi.ptr(x), m, _ffi.ptr(dist), GAUSS["offset"], _ffi.ptr(ft["tables"][i]),
                          ctypes.byref(lay), _ffi.ptr(recv), _ffi.ptr(send), None, m, 0, 0, _ffi.ptr(out), None, 0,
                          _ffi.stream())
            torch.cuda.synchronize()
            res[name] = float(np.max(np.abs(out.cpu().numpy().astype(np.float64) - ref))) / scale
        print("block %d: scale %.4f; against float64 on %d check distances: MFMA kernel %.3e, table kernel %.3e, "
              "build's self-check %.3e (bar %.2e)" % (i, scale, m, res["mfma"], res["table"], ft["err"][i],
                                                      fused.FILTER_TABLE_BAR))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        fused.pack_weights(pd, 3, GAUSS["bins"], out=images)
    t_all = (time.perf_counter() - t0) / 10
    del images["ftable"]
    images["ftable"] = None
    t0 = time.perf_counter()
    for _ in range(10):
        fused.pack_weights(pd, 3, GAUSS["bins"], out=images)
    t_without = (time.perf_counter() - t0) / 10
    print("weight update: pack_weights %.0f us with the three tables, %.0f us without" % (t_all * 1e6, t_without * 1e6))
    images["ftable"] = ft

    rng = np.random.default_rng(0)
    for tiles in (4093, 819):
        m = tiles * 32 - 7
        n = m // 11
        r = np.sort(rng.integers(0, n, size=m)).astype(np.int32)
        s = np.clip(r + rng.integers(-18, 19, size=m), 0, n - 1).astype(np.int32)
        xx = torch.randn((n, F), device="cuda")
        dd = dev(rng.uniform(0.9, 4.0, size=m).astype(f32))
        rr, ss = dev(r), dev(s)
        out = torch.zeros((n, F), dtype=torch.float32, device="cuda")
        row = ["%d tiles:" % tiles]
        for waves in (4, 8, 16):
            us = timed(lambda: _ffi.call("mp_cfconv_table_f32", _ffi.ptr(xx), n, _ffi.ptr(dd), 0.0,
                                         _ffi.ptr(ft["tables"][0]), ctypes.byref(lay), _ffi.ptr(rr), _ffi.ptr(ss), None, m,
                                         0, waves, _ffi.ptr(out), None, 0, _ffi.stream()))
            row.append("table %d waves %.1f us" % (waves, us))
        us = timed(lambda: _ffi.call("mp_cfconv_gauss_fused_f32", _ffi.ptr(xx), n, _ffi.ptr(dd), GAUSS["bins"],
                                     GAUSS["distance"], GAUSS["sigma"], GAUSS["offset"], _ffi.ptr(images["cfconv"][0]),
                                     _ffi.ptr(rr), _ffi.ptr(ss), None, m, 1, _ffi.ptr(out), _ffi.stream()))
        row.append("MFMA kernel %.1f us (launches issued back to back through ctypes)" % us)
        print("  ".join(row))


if __name__ == "__main__":
    main()
