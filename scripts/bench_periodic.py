"""Periodic cells: the on-GPU ``SetRangePeriodic`` and the crystal SchNet on its result, on the 128 structures of
``synth.periodic_structures`` (4-30 atoms, about 0.07 atoms per cubic Angstrom, skewed cells).

Steps (HIP events, median of --steps calls after --warmup calls):

* ``search_c4`` / ``search_c5``: the whole ``SetRangePeriodic`` call at cutoff 4 / 5 (count, the one host read, allocation,
  fill) and its two engine calls alone;
* ``set_range``: the molecular ``SetRange`` (cutoff 5, every neighbour) on the same coordinates read as molecules - a batch
  of equal ``N`` as yardstick;
* ``schnet_forward`` / ``schnet_energy_force``: the crystal SchNet (default configuration) on the cutoff-4 edges, replayed
  forward and ``EnergyForceModel`` on the tape.

Every step runs in a child process of its own under its own time limit; the first step that fails or runs out of time
ends the run (nothing more is started on the device).  Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys

STEPS = ["search_c4", "search_c5", "set_range", "schnet_forward", "schnet_energy_force"]
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


def run_step(step, args):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from gcnn_keras_amd import _ffi, synth
    from gcnn_keras_amd.graph.preprocessor import SetRange, SetRangePeriodic
    from gcnn_keras_amd.ragged import RaggedTensor
    if not torch.cuda.is_available():
        raise SystemExit("bench_periodic.py needs an MI355X: no device, no timing")
    b = synth.periodic_structures(args.graphs)
    xyz = RaggedTensor.from_numpy(b["node_coordinates"], b["node_splits"])
    lattice = torch.from_numpy(b["graph_lattice"]).cuda()
    n, g = int(b["node_splits"][-1]), args.graphs
    res = {"graphs": g, "atoms": n}
    if step in ("search_c4", "search_c5"):
        cutoff = 4.0 if step == "search_c4" else 5.0
        sp = SetRangePeriodic(max_distance=cutoff)
        idx, _, _ = sp(xyz, lattice)
        m = int(idx.values.shape[0])
        deg = (idx.index_plan(xyz).csr(0)[0][1:] - idx.index_plan(xyz).csr(0)[0][:-1]).cpu().numpy()
        res.update({"cutoff": cutoff, "edges": m, "max_degree": int(deg.max()),
                    "call_ms": timed(lambda: sp(xyz, lattice), args.steps, args.warmup)})
        nbytes = _ffi.workspace_bytes("mp_radius_graph_periodic_workspace_bytes", n)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
        head = torch.empty(n + 2, dtype=torch.int32, device="cuda")
        es = torch.empty(g + 1, dtype=torch.int64, device="cuda")
        out = [torch.empty((m, 2), dtype=torch.int64, device="cuda"), torch.empty((m, 3), dtype=torch.int64, device="cuda"),
               torch.empty((2, m), dtype=torch.int32, device="cuda"), torch.empty((m, 1), dtype=torch.float32, device="cuda")]
        x, sx = xyz.values, xyz.row_splits

        def count():
            _ffi.call("mp_radius_graph_periodic_count_f32", _ffi.ptr(x), _ffi.ptr(sx), _ffi.ptr(lattice), g, n, cutoff, -1,
                      _ffi.ptr(head[:n + 1]), _ffi.ptr(es), _ffi.ptr(head[n + 1:]), _ffi.ptr(ws), nbytes, _ffi.stream())

        def fill():
            _ffi.call("mp_radius_graph_periodic_fill_f32", _ffi.ptr(x), _ffi.ptr(sx), _ffi.ptr(lattice), g, n, cutoff, -1,
                      _ffi.ptr(head[:n + 1]), m, _ffi.ptr(out[0]), _ffi.ptr(out[1]), _ffi.ptr(out[2][0]),
                      _ffi.ptr(out[2][1]), _ffi.ptr(out[3]), _ffi.stream())

        res["count_ms"] = timed(count, args.steps, args.warmup)
        res["fill_ms"] = timed(fill, args.steps, args.warmup)
    elif step == "set_range":
        sr = SetRange(max_distance=5.0, max_neighbours=10000)
        idx, _ = sr(xyz)
        res.update({"cutoff": 5.0, "edges": int(idx.values.shape[0]),
                    "call_ms": timed(lambda: sr(xyz), args.steps, args.warmup)})
    else:
        from gcnn_keras_amd.literature import Schnet
        from gcnn_keras_amd.model.force import EnergyForceModel
        idx, img, _ = SetRangePeriodic(max_distance=4.0)(xyz, lattice)
        model = Schnet.make_crystal_model(inputs=Schnet.model_crystal_default["inputs"])
        model.set_weights(list(synth.schnet_params(seed=7, depth=4, random_bias=True).values()))
        inputs = [RaggedTensor.from_numpy(b["node_number"], b["node_splits"]), xyz, idx, img, lattice]
        res["edges"] = int(idx.values.shape[0])
        if step == "schnet_forward":
            model(inputs), model(inputs)
            res["forward_ms"] = timed(lambda: model(inputs), args.steps, args.warmup)
            res["route"] = model.last_route
        else:
            efm = EnergyForceModel(model_energy=model, coordinate_input=1, energy_output=0, output_as_dict=True,
                                   output_to_tensor=False, output_squeeze_states=True)
            res["energy_force_ms"] = timed(lambda: efm(inputs), args.steps, args.warmup)
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
