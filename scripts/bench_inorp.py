"""INorp on 128 molecule-like graphs of ``synth.cmpnn_batch`` (about 1 600 atoms, 3 500 directed edges) with the ESOL
configuration of the reference's training suite (41 node and 11 edge features, the graph state embedded, edge and node
MLPs [32, 32], depth 3, sum pooling).

Steps (HIP events, median of --steps calls after --warmup calls):

* ``forward``: the whole model on the fused route (``INorpEdgeStep``: three node-sized Dense launches around
  ``mp_inorp_edge_f32``) against the layer sequence (``use_fused_step = False``: the reference's op sequence), eager and
  replayed from a HIP graph each; engine calls per forward on both routes;
* ``train``: one ``train_on_batch`` step (SGD, mean absolute error) on the fused tape (``autograd.InorpEdge``) against the
  layer sequence's tape; engine calls of one forward + backward on both routes.

Both routes are measured twice, alternated (fused, layer sequence, fused, layer sequence): every figure is a list of two.
The tree before INorp has no such model, so the baseline is the layer sequence of this tree.

Every step runs in a child process of its own under its own time limit; the first step that fails or runs out of time
ends the run (nothing more is started on the device).  Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys

STEPS = ["forward", "train"]
STEP_LIMIT_S = 120
ROUTES = ((True, "fused"), (False, "layer_sequence")) * 2

ESOL = {
    "inputs": [{"shape": [None, 41], "name": "node_attributes", "dtype": "float32", "ragged": True},
               {"shape": [None, 11], "name": "edge_attributes", "dtype": "float32", "ragged": True},
               {"shape": [None, 2], "name": "edge_indices", "dtype": "int64", "ragged": True},
               {"shape": [], "name": "graph_size", "dtype": "float32", "ragged": False}],
    "input_embedding": {"node": {"input_dim": 95, "output_dim": 32}, "edge": {"input_dim": 15, "output_dim": 32},
                        "graph": {"input_dim": 32, "output_dim": 32}},
    "node_mlp_args": {"units": [32, 32], "use_bias": True, "activation": ["relu", "linear"]},
    "edge_mlp_args": {"units": [32, 32], "activation": ["relu", "linear"]},
    "pooling_args": {"pooling_method": "segment_sum"}, "depth": 3, "verbose": 30,
    "output_mlp": {"use_bias": [True, True, False], "units": [32, 32, 1], "activation": ["relu", "relu", "linear"]},
}


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
    from gcnn_keras_amd.literature import INorp
    from gcnn_keras_amd.ragged import RaggedTensor
    if not torch.cuda.is_available():
        raise SystemExit("bench_inorp.py needs an MI355X: no device, no timing")
    b = synth.cmpnn_batch(args.graphs, node_features=41, edge_features=11)
    ns, es = b["node_splits"], b["edge_splits"]
    rag = lambda v, s: RaggedTensor.from_numpy(np.ascontiguousarray(v), s)
    res = {"graphs": args.graphs, "atoms": int(ns[-1]), "edges": int(es[-1])}
    m = INorp.make_model(**ESOL)
    m.set_weights(parity_weights(m))
    res["fused_step_rounds"] = m.fused_step_rounds
    state = torch.from_numpy(np.random.default_rng(7).integers(0, 16, size=args.graphs).astype(np.float32)).cuda()
    x = [rag(b["node_attributes"], ns), rag(b["edge_attributes"], es), rag(b["edge_indices"], es), state]

    def add(key, value):
        res.setdefault(key, []).append(value)
    if step == "forward":
        with torch.no_grad():
            for fused, key in ROUTES:
                m.use_fused_step = fused
                m.auto_graph = False
                m(x)
                before = _ffi.launch_count()
                m(x)
                add("launches_" + key, _ffi.launch_count() - before)
                add("eager_%s_ms" % key, timed(lambda: m(x), args.steps, args.warmup))
                # flipping the switch released the captured graphs: each route is captured, then timed on its own graph
                m.auto_graph = True
                m.release_graphs()
                m(x), m(x), m(x)
                add("replayed_%s_ms" % key, timed(lambda: m(x), args.steps, args.warmup))
                add("route_" + key, m.last_route)
    else:
        target = np.random.default_rng(6).uniform(-1.0, 1.0, size=(args.graphs, 1)).astype(np.float32)
        m.compile(optimizer=torch.optim.SGD(m.trainable_weights, lr=1e-3), loss="mean_absolute_error")
        for fused, key in ROUTES:
            m.use_fused_step = fused
            m.train_on_batch(x, target)
            before = _ffi.launch_count()
            add("loss_" + key, float(m.train_on_batch(x, target)))
            add("launches_" + key, _ffi.launch_count() - before)
            add("train_%s_ms" % key, timed(lambda: m.train_on_batch(x, target), args.steps, args.warmup))
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
