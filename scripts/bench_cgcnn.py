"""CGCNN on the 128 structures of ``synth.periodic_structures`` (4-30 atoms, about 0.07 atoms per cubic Angstrom, skewed
cells), edges from the on-GPU ``SetRangePeriodic`` at cutoff 5: cut after 12 neighbours (the usual CGCNN setting) and
uncut (about 78 000 edges, 35-45 per receiver).

Steps (HIP events, median of --steps calls after --warmup calls, the two routes alternated call by call):

* ``layer_n12`` / ``layer_uncut``: one ``CGCNNLayer`` (64 units, 40 Gauss features, batch normalisation on) - the fused
  ``mp_cgcnn_gate_f32`` (four node-side Dense + one kernel + the update pass) against the reference's layer sequence
  (gather, concatenate, two Dense, two batch norms, two activations, multiply, PoolingLocalEdges, batch norm, add,
  activation), eager;
* ``model_n12`` / ``model_uncut``: the whole default model (depth 3, geometry included) replayed from its HIP graph,
  with and without the fused step.

Every step runs in a child process of its own under its own time limit; the first step that fails or runs out of time
ends the run (nothing more is started on the device).  Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys

STEPS = ["layer_n12", "layer_uncut", "model_n12", "model_uncut"]
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
    from gcnn_keras_amd import synth
    from gcnn_keras_amd.graph.preprocessor import SetRangePeriodic
    from gcnn_keras_amd.layers.conv.cgcnn_conv import CGCNNLayer
    from gcnn_keras_amd.layers.geom import GaussBasisLayer
    from gcnn_keras_amd.literature import CGCNN
    from gcnn_keras_amd.ragged import RaggedTensor
    if not torch.cuda.is_available():
        raise SystemExit("bench_cgcnn.py needs an MI355X: no device, no timing")
    b = synth.cgcnn_batch(synth.periodic_structures(args.graphs))
    xyz = RaggedTensor.from_numpy(b["node_coordinates"], b["node_splits"])
    kind, cut = step.split("_")
    search = SetRangePeriodic(max_distance=5.0, max_neighbours=12) if cut == "n12" else SetRangePeriodic(max_distance=5.0)
    idx, img, dist = search(xyz, torch.from_numpy(b["graph_lattice"]).cuda())
    n, e = int(b["node_splits"][-1]), int(idx.values.shape[0])
    res = {"graphs": args.graphs, "atoms": n, "edges": e}
    with torch.no_grad():
        if kind == "layer":
            rng = np.random.default_rng(0)
            lay = CGCNNLayer(units=64, batch_normalization=True)
            lay.ensure_built([(None, None, 64), (None, None, 40), (None, None, 2)])
            lay.set_weights([rng.uniform(0.5, 1.5, w.shape).astype(np.float32) if w.ndim == 1 else
                             synth.glorot_uniform(rng, w.shape[0], w.shape[1], shape=w.shape) for w in lay.get_weights()])
            h = xyz.with_values(torch.from_numpy(rng.normal(size=(n, 64)).astype(np.float32)).cuda())
            feats = GaussBasisLayer(bins=40, distance=8, sigma=0.4)(dist)

            def call(fused):
                lay.use_fused_gate = fused
                return lay([h, feats, idx])

            call(True), call(False)      # build the plan and its CSRs outside the timed calls
            res["fused_ms"], res["layer_sequence_ms"] = timed_pair(lambda: call(True), lambda: call(False), args.steps,
                                                                   args.warmup)
        else:
            m = CGCNN.make_crystal_model()
            m.set_weights(list(synth.cgcnn_params(m).values()))
            x = [RaggedTensor.from_numpy(b["node_number"], b["node_splits"]),
                 RaggedTensor.from_numpy(b["node_frac_coordinates"], b["node_splits"]), idx,
                 torch.from_numpy(b["lattice_matrix"]).cuda(), img]
            # flipping the switch releases the captured graphs: each route is captured, then timed on its own graph
            for fused, key in ((True, "fused_ms"), (False, "layer_sequence_ms")):
                m.use_fused_gate = fused
                m(x), m(x), m(x)
                res[key] = timed(lambda: m(x), args.steps, args.warmup)
                res["route_" + key[:-3]] = m.last_route
        res["speedup"] = res["layer_sequence_ms"] / res["fused_ms"]
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
