"""MAT on 128 molecule graphs of ``synth.mat_batch`` (about 1 600 atoms, 3 500 directed bonds), default model (depth 5,
8 heads of 8 units, width 32).

Steps (HIP events, median of --steps calls after --warmup calls):

* ``fused``: every attention sub-block on ``FusedMATBlock`` (layer normalisation, one packed q|k|v ``Dense``, one
  ``mp_mat_attention_f32`` with the merge + residual epilogue), eager and replayed from a HIP graph; engine calls per forward;
* ``layers``: the layer sequence (``use_fused_attention = False``: per head three ``Dense`` and one attention launch, the
  concatenation, the merging ``Dense``, the residual add), eager and replayed; engine calls per forward;
* ``torch``: the padded restatement of tests/mat_reference.py (``forward_padded``: what a user would write in PyTorch,
  the reference's op sequence with its ``(batch, Nmax, Nmax, units)`` score tensors) on the same device, eager, the inputs
  padded beforehand (padding is not timed); and its largest difference from the fused route.

The parent of this model cannot run MAT, so there is no earlier time to hold these to.

Every step runs in a child process of its own under its own time limit; the first step that fails or runs out of time
ends the run (nothing more is started on the device).  Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys

STEPS = ["fused", "layers", "torch"]
STEP_LIMIT_S = 120
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def run_step(step, args):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from gcnn_keras_amd import _ffi, synth
    from gcnn_keras_amd.literature import MAT
    from gcnn_keras_amd.ragged import RaggedTensor
    if not torch.cuda.is_available():
        raise SystemExit("bench_mat.py needs an MI355X: no device, no timing")
    b = synth.mat_batch(args.graphs)
    ns, es = b["node_splits"], b["edge_splits"]
    rag = lambda v, s: RaggedTensor.from_numpy(np.ascontiguousarray(v), s)
    res = {"graphs": args.graphs, "atoms": int(ns[-1]), "edges": int(es[-1]), "largest": int(np.diff(ns).max())}
    m = MAT.make_model(verbose=30)
    params = synth.mat_params(m)
    m.set_weights(list(params.values()))
    x = [rag(b["node_number"], ns), rag(b["node_coordinates"], ns), rag(b["edge_weights"], es), rag(b["edge_indices"], es)]
    with torch.no_grad():
        if step in ("fused", "layers"):
            m.use_fused_attention = step == "fused"
            res["fused_attention_blocks"] = m.fused_attention_blocks
            m.auto_graph = False
            m(x)
            before = _ffi.launch_count()
            m(x)
            res["launches"] = _ffi.launch_count() - before
            res["eager_ms"] = timed(lambda: m(x), args.steps, args.warmup)
            m.auto_graph = True
            m.release_graphs()
            m(x), m(x), m(x)
            res["replayed_ms"] = timed(lambda: m(x), args.steps, args.warmup)
            res["route"] = m.last_route
        else:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import mat_reference as mref
            cfg = mref.config()
            p = {k: torch.from_numpy(v).cuda() for k, v in zip(mref.model_params(np.random.default_rng(0), cfg),
                                                               params.values())}
            inputs = mref.padded_inputs(cfg, b, torch.float32, device="cuda")
            res["torch_padded_eager_ms"] = timed(lambda: mref.forward_padded(p, cfg, inputs), args.steps, args.warmup)
            got, want = m(x), mref.forward_padded(p, cfg, inputs)
            res["max_abs_diff_fused_vs_torch"] = float((got - want).abs().max())
            res["max_abs_output"] = float(want.abs().max())
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
