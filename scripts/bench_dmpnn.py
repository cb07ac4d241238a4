"""DMPNN on 128 molecule-like graphs of ``synth.cmpnn_batch`` (about 1 600 atoms, 3 500 directed edges), default model
(width 128, depth 5, embeddings).

Steps (HIP events, median of --steps calls after --warmup calls):

* ``forward``: the whole default model, fused rounds (``DMPNNStep``: the receiver sum and ``mp_directed_edge_update_f32``)
  against the layer sequence (``use_fused_step = False`` - the route every configuration had before), eager and replayed
  from a HIP graph each; engine calls per forward on both routes;
* ``train``: one ``train_on_batch`` step (SGD, mean squared error) on the fused tape (``autograd.DirectedEdgeUpdate``,
  csrc/mp_dmpnn.hip) against the layer sequence's tape; engine calls of one forward + backward on both routes.

On a tree whose DMPNN has no ``use_fused_step`` switch (before the fused round) the script measures the one route there
is and reports it as ``layer_sequence``.

Every step runs in a child process of its own under its own time limit; the first step that fails or runs out of time
ends the run (nothing more is started on the device).  Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys

STEPS = ["forward", "train"]
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


def parity_weights(model, seed=41):
    """Dense kernels Glorot-uniform times 0.5, biases in +-0.1, embeddings in +-0.5 (the weights of the parity tests)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    out = []
    for name, t in model.weights:
        shape = tuple(int(s) for s in t.shape)
        leaf = name.rsplit("/", 1)[-1]
        if leaf == "embeddings":
            v = rng.uniform(-0.5, 0.5, size=shape)
        elif leaf == "bias":
            v = rng.uniform(-0.1, 0.1, size=shape)
        else:
            v = 0.5 * rng.uniform(-1.0, 1.0, size=shape) * np.sqrt(6.0 / (shape[0] + shape[-1]))
        out.append(np.asarray(v, dtype=np.float32))
    return out


def run_step(step, args):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from gcnn_keras_amd import _ffi, synth
    from gcnn_keras_amd.literature import DMPNN
    from gcnn_keras_amd.ragged import RaggedTensor
    if not torch.cuda.is_available():
        raise SystemExit("bench_dmpnn.py needs an MI355X: no device, no timing")
    b = synth.cmpnn_batch(args.graphs)
    ns, es = b["node_splits"], b["edge_splits"]
    rag = lambda v, s: RaggedTensor.from_numpy(np.ascontiguousarray(v), s)
    res = {"graphs": args.graphs, "atoms": int(ns[-1]), "edges": int(es[-1])}
    m = DMPNN.make_model(verbose=30)
    m.set_weights(parity_weights(m))
    x = [rag(b["node_number"].astype(np.float32), ns), rag(b["edge_number"].astype(np.float32), es),
         rag(b["edge_indices"], es), rag(b["edge_indices_reverse"], es)]
    switch = hasattr(m, "use_fused_step")
    res["has_fused_step"] = switch
    routes = ((True, "fused"), (False, "layer_sequence")) if switch else ((False, "layer_sequence"),)
    if step == "forward":
        with torch.no_grad():
            for fused, key in routes:
                if switch:
                    m.use_fused_step = fused
                m.auto_graph = False
                m(x)
                before = _ffi.launch_count()
                m(x)
                res["launches_" + key] = _ffi.launch_count() - before
                res["eager_%s_ms" % key] = timed(lambda: m(x), args.steps, args.warmup)
                # flipping the switch released the captured graphs: each route is captured, then timed on its own graph
                m.auto_graph = True
                m.release_graphs()
                m(x), m(x), m(x)
                res["replayed_%s_ms" % key] = timed(lambda: m(x), args.steps, args.warmup)
                res["route_" + key] = m.last_route
    else:
        target = np.random.default_rng(6).uniform(-1.0, 1.0, size=(args.graphs, 1)).astype(np.float32)
        m.compile(optimizer=torch.optim.SGD(m.trainable_weights, lr=1e-3), loss="mean_squared_error")
        for fused, key in routes:
            if switch:
                m.use_fused_step = fused
            m.train_on_batch(x, target)
            before = _ffi.launch_count()
            res["loss_" + key] = float(m.train_on_batch(x, target))
            res["launches_" + key] = _ffi.launch_count() - before
            res["train_%s_ms" % key] = timed(lambda: m.train_on_batch(x, target), args.steps, args.warmup)
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
