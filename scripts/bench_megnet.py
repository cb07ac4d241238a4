"""MEGNet's crystal model on structures of ``synth.periodic_structures`` (4-30 atoms, about 0.07 atoms per cubic Angstrom,
skewed cells), edges from the on-GPU ``SetRangePeriodic`` at cutoff 5 (uncut: 35-45 edges per atom): the default
``Megnet.make_crystal_model`` forward with the fused edge step (``mp_megnet_edge_f32``) against the layer sequence
(``use_fused_edge=False``: the reference's op sequence, one engine call per layer).

Steps (HIP events, median of --steps calls after --warmup calls, the two routes alternated call by call):

* ``batch64``: one batch of 64 structures - eager and replayed from the model's HIP graph;
* ``single``: one structure - eager and replayed;
* ``molecular``: the default ``Megnet.make_model`` on 128 QM9-shaped molecules, both routes, eager and replayed.

Every step also times one ``MEGnetBlock`` call (32-wide random features on the step's graph, eager) on either route and
reports the engine calls of one eager forward and of one ``MEGnetBlock`` call on either route
(``_ffi.launch_count``).  Every step runs in a child process of its own under its own time limit; the first step that
fails or runs out of time ends the run (nothing more is started on the device).  Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys

STEPS = ["batch64", "single", "molecular"]
STEP_LIMIT_S = 150


def _event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


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
    from gcnn_keras_amd.graph.preprocessor import SetRangePeriodic
    from gcnn_keras_amd.literature import Megnet
    from gcnn_keras_amd.ragged import RaggedTensor
    if not torch.cuda.is_available():
        raise SystemExit("bench_megnet.py needs an MI355X: no device, no timing")
    rng = np.random.default_rng(0)
    rag = RaggedTensor.from_numpy
    if step == "molecular":
        b = synth.qm9_like_batch(num_graphs=128)
        g = len(b["node_splits"]) - 1
        m = Megnet.make_model()
        idx = rag(b["edge_indices"], b["edge_splits"])
        x = [rag(b["node_number"], b["node_splits"]), rag(b["node_coordinates"], b["node_splits"]), idx,
             torch.from_numpy(rng.integers(0, 100, size=g).astype(np.float32)).cuda()]
    else:
        b = synth.periodic_structures(64 if step == "batch64" else 1)
        g = len(b["node_splits"]) - 1
        m = Megnet.make_crystal_model()
        xyz, lattice = rag(b["node_coordinates"], b["node_splits"]), torch.from_numpy(b["graph_lattice"]).cuda()
        idx, img, _ = SetRangePeriodic(max_distance=5.0)(xyz, lattice)
        x = [rag(b["node_number"].astype(np.float32), b["node_splits"]), xyz, idx,
             torch.from_numpy(rng.normal(size=(g, 1)).astype(np.float32)).cuda(), img, lattice]
    m.set_weights(list(synth.cgcnn_params(m, seed=7).values()))
    n, e = int(b["node_splits"][-1]), int(idx.values.shape[0])
    res = {"graphs": g, "atoms": n, "edges": e, "fused_edge_blocks": m.fused_edge_blocks}

    def call(fused):
        # the per-block switch: both routes keep their captured graph (the switch is part of the graph key)
        for blk in m.blocks:
            blk.use_fused_edge = fused
        return m(x)

    def launches(fn):
        before = _ffi.launch_count()
        fn()
        return _ffi.launch_count() - before

    with torch.no_grad():
        m.auto_graph = False
        call(True), call(False)          # build the plan and its CSRs outside the counted and timed calls
        res["forward_calls_fused"], res["forward_calls_layer_sequence"] = launches(lambda: call(True)), \
            launches(lambda: call(False))
        blk = m.blocks[0]
        feats = [x[0].with_values(torch.from_numpy(rng.normal(size=(n, 32)).astype(np.float32)).cuda()),
                 idx.with_values(torch.from_numpy(rng.normal(size=(e, 32)).astype(np.float32)).cuda()), idx,
                 torch.from_numpy(rng.normal(size=(g, 32)).astype(np.float32)).cuda()]
        for fused, key in ((True, "block_calls_fused"), (False, "block_calls_layer_sequence")):
            blk.use_fused_edge = fused
            blk(feats)
            res[key] = launches(lambda: blk(feats))

        def block_call(fused):
            blk.use_fused_edge = fused
            return blk(feats)

        res["block_fused_ms"], res["block_layer_sequence_ms"] = timed_pair(lambda: block_call(True),
                                                                           lambda: block_call(False), args.steps,
                                                                           args.warmup)
        res["eager_fused_ms"], res["eager_layer_sequence_ms"] = timed_pair(lambda: call(True), lambda: call(False),
                                                                           args.steps, args.warmup)
        m.auto_graph = True
        for fused in (True, False):
            call(fused), call(fused), call(fused)
            res["route_fused" if fused else "route_layer_sequence"] = m.last_route
        res["replay_fused_ms"], res["replay_layer_sequence_ms"] = timed_pair(lambda: call(True), lambda: call(False),
                                                                             args.steps, args.warmup)
    res["eager_speedup"] = res["eager_layer_sequence_ms"] / res["eager_fused_ms"]
    res["replay_speedup"] = res["replay_layer_sequence_ms"] / res["replay_fused_ms"]
    res["block_speedup"] = res["block_layer_sequence_ms"] / res["block_fused_ms"]
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--step", choices=STEPS, default=None, help="run this one step in this process")
    args = ap.parse_args()
    if args.step is not None:
        run_step(args.step, args)
        return
    res = {"steps": args.steps, "warmup": args.warmup}
    for step in STEPS:
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--step", step,
               "--steps", str(args.steps), "--warmup", str(args.warmup)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if done.returncode != 0:
            res["failed"] = {"step": step, "returncode": done.returncode}
            print(json.dumps(res))
            raise SystemExit(1)
        res[step] = json.loads(done.stdout.strip().splitlines()[-1])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
