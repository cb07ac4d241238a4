"""CMPNN on 128 molecule-like graphs of ``synth.cmpnn_batch`` (about 1 600 atoms, 3 500 directed edges), default model
(width 300, depth 5, GRU readout).

Steps (HIP events, median of --steps calls after --warmup calls):

* ``round``: one ``CMPNNCommunicate`` - the two fused launches (``mp_cmpnn_boost_f32``, ``mp_directed_edge_update_f32``)
  against the reference's layer sequence, eager (the two routes alternated call by call) and replayed from a HIP graph
  each; engine calls per round on both routes;
* ``model``: the whole default model, fused rounds against the layer sequence (``use_fused_communicate = False`` - the
  route every configuration had before the fused kernels), eager and replayed;
* ``gru``: the readout's recurrence ``mp_gru_ragged_last_f32`` alone (the input GEMM outside) and the whole layer.

Every step runs in a child process of its own under its own time limit; the first step that fails or runs out of time
ends the run (nothing more is started on the device).  Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys

STEPS = ["round", "model", "gru"]
STEP_LIMIT_S = 120


def _event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed(fn, steps, warmup):
    import numpy as np
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return float(np.median([_event_ms(fn) for _ in range(steps)]))


def timed_pair(fn_a, fn_b, steps, warmup):
    """Medians of two calls alternated a, b, a, b, ... (same clocks, same caches for both)."""
    import numpy as np
    import torch
    for _ in range(warmup):
        fn_a()
        fn_b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(steps):
        ta.append(_event_ms(fn_a))
        tb.append(_event_ms(fn_b))
    return float(np.median(ta)), float(np.median(tb))


def run_step(step, args):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from gcnn_keras_amd import _ffi, synth
    from gcnn_keras_amd.layers.conv.cmpnn_conv import CMPNNCommunicate
    from gcnn_keras_amd.layers.modules import _dense_raw
    from gcnn_keras_amd.layers.pool.gru import PoolingNodesGRU
    from gcnn_keras_amd.literature import CMPNN
    from gcnn_keras_amd.model.utils import Model
    from gcnn_keras_amd.ragged import RaggedTensor
    if not torch.cuda.is_available():
        raise SystemExit("bench_cmpnn.py needs an MI355X: no device, no timing")
    b = synth.cmpnn_batch(args.graphs)
    ns, es = b["node_splits"], b["edge_splits"]
    n, e = int(ns[-1]), int(es[-1])
    rng = np.random.default_rng(0)
    rag = lambda v, s: RaggedTensor.from_numpy(np.ascontiguousarray(v), s)
    res = {"graphs": args.graphs, "atoms": n, "edges": e}
    with torch.no_grad():
        if step == "round":
            width = 300
            lay = CMPNNCommunicate(edge_dense={"units": width, "activation": "linear"},
                                   edge_activation={"activation": "relu"}, pooling_kwargs={"pooling_method": "sum"},
                                   dropout={"rate": 0.1})
            lay.ensure_built([(None, None, width)] * 3 + [(None, None, 2), (None, None, 1)])
            lay.set_weights([0.5 * synth.glorot_uniform(rng, width, width),
                             rng.uniform(-0.1, 0.1, width).astype(np.float32)])
            ev = (0.3 * rng.normal(size=(e, width))).astype(np.float32)
            x = [rag((0.3 * rng.normal(size=(n, width))).astype(np.float32), ns), rag(ev, es), rag(ev, es),
                 rag(b["edge_indices"], es), rag(b["edge_indices_reverse"], es)]

            def call(fused):
                lay.use_fused_communicate = fused
                return lay(x)

            call(True), call(False)      # build the plans and their CSR outside the timed calls
            for fused, key in ((True, "fused"), (False, "layer_sequence")):
                before = _ffi.launch_count()
                call(fused)
                res["launches_" + key] = _ffi.launch_count() - before
            res["eager_fused_ms"], res["eager_layer_sequence_ms"] = timed_pair(lambda: call(True), lambda: call(False),
                                                                              args.steps, args.warmup)
            for fused, key in ((True, "fused"), (False, "layer_sequence")):
                lay.use_fused_communicate = fused
                m = Model("round", lambda inputs: lay(inputs), [lay], auto_graph=True)
                m(x), m(x), m(x)
                res["replayed_%s_ms" % key] = timed(lambda: m(x), args.steps, args.warmup)
                res["route_" + key] = m.last_route
        elif step == "model":
            m = CMPNN.make_model(verbose=30)
            m.set_weights(list(synth.cmpnn_params(m).values()))
            x = [rag(b["node_number"].astype(np.float32), ns), rag(b["edge_number"].astype(np.float32), es),
                 rag(b["edge_indices"], es), rag(b["edge_indices_reverse"], es)]
            for fused, key in ((True, "fused"), (False, "layer_sequence")):
                m.use_fused_communicate = fused
                m.auto_graph = False
                m(x)
                before = _ffi.launch_count()
                m(x)
                res["launches_" + key] = _ffi.launch_count() - before
                res["eager_%s_ms" % key] = timed(lambda: m(x), args.steps, args.warmup)
                # flipping the switch released the captured graphs: each route is captured, then timed on its own graph
                m.auto_graph = True
                m(x), m(x), m(x)
                res["replayed_%s_ms" % key] = timed(lambda: m(x), args.steps, args.warmup)
                res["route_" + key] = m.last_route
        else:
            units = 300
            lay = PoolingNodesGRU(units=units)
            lay.ensure_built((None, None, units))
            lay.set_weights([synth.glorot_uniform(rng, units, 3 * units), synth.glorot_uniform(rng, units, 3 * units),
                             rng.uniform(-0.1, 0.1, (2, 3 * units)).astype(np.float32)])
            x = rag((0.3 * rng.normal(size=(n, units))).astype(np.float32), ns)
            res["longest_graph"] = int(np.max(np.diff(ns)))
            mx = _dense_raw(x.values, lay.kernel, lay.bias[0].contiguous(), 0, 0.0)
            out = torch.empty((args.graphs, units), dtype=torch.float32, device="cuda")
            b_rec = lay.bias[1].contiguous()

            def recurrence():
                _ffi.call("mp_gru_ragged_last_f32", _ffi.ptr(mx), n, _ffi.ptr(x.row_splits), args.graphs,
                          _ffi.ptr(lay.recurrent_kernel), _ffi.ptr(b_rec), units, lay._act, lay._rec, _ffi.ptr(out),
                          _ffi.stream())

            res["recurrence_ms"] = timed(recurrence, args.steps, args.warmup)
            res["layer_ms"] = timed(lambda: lay(x), args.steps, args.warmup)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--graphs", type=int, default=128)
    ap.add_argument("--step", choices=STEPS, default=None, help="run this one step in this process")
    args = ap.parse_args()
    if args.step is not None:
        run_step(args.step, args)
        return
    res = {"steps": args.steps, "warmup": args.warmup}
    for step in STEPS:
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", step,
               "--steps", str(args.steps), "--warmup", str(args.warmup), "--graphs", str(args.graphs)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if done.returncode != 0:
            res["failed"] = {"step": step, "returncode": done.returncode}
            print(json.dumps(res))
            raise SystemExit(1)
        res[step] = json.loads(done.stdout.strip().splitlines()[-1])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
