"""HDNNP2nd at the fork's configuration (force_hdnnp2nd.py:43-65, 139-204): 128 alanine-dipeptide-shaped molecules.

Times (median of HIP events, per call): the energy forward (eager layer path and the replayed auto-graph), energy +
forces on the inference tape (``EnergyForceModel``, is_physical_force=False), and one ``EnergyForceModel.train_on_batch``
step (Adam, clipnorm 1.0, MSE losses weighted [1/200, 199/200]).  Prints one JSON line.  A kernel breakdown:
``rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_hdnnp.py --only train --steps 5``."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gcnn_keras_amd import synth                        # noqa: E402
from gcnn_keras_amd.literature import HDNNP2nd          # noqa: E402
from gcnn_keras_amd.model.force import EnergyForceModel  # noqa: E402
from gcnn_keras_amd.ragged import RaggedTensor          # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["all", "forward", "force", "train"], default="all")
    args = ap.parse_args()
    b = synth.hdnnp_batch(num_graphs=args.graphs, seed=3456)
    inputs = [RaggedTensor.from_numpy(b["node_number"], b["node_splits"]),
              RaggedTensor.from_numpy(b["node_coordinates"], b["node_splits"]),
              RaggedTensor.from_numpy(b["edge_indices"], b["edge_splits"]),
              RaggedTensor.from_numpy(b["angle_indices"], b["angle_splits"])]
    model = HDNNP2nd.make_model_behler(**synth.hdnnp_model_kwargs())
    model.set_weights(list(synth.hdnnp_params().values()))
    efm = EnergyForceModel(model_energy=model, energy_output=0, output_as_dict=False, output_squeeze_states=True,
                           is_physical_force=False)
    res = {"graphs": args.graphs, "atoms": int(b["node_splits"][-1]), "edges": int(b["edge_splits"][-1]),
           "triplets": int(b["angle_splits"][-1]), "steps": args.steps}
    if args.only in ("all", "forward"):
        model.auto_graph = False
        res["forward_eager_ms"] = timed(lambda: model(inputs), args.steps, args.warmup)
        model.auto_graph = True
        res["forward_replayed_ms"] = timed(lambda: model(inputs), args.steps, args.warmup)
    if args.only in ("all", "force"):
        res["energy_force_ms"] = timed(lambda: efm(inputs), args.steps, args.warmup)
    if args.only in ("all", "train"):
        efm.compile(optimizer="adam", loss=["mean_squared_error", "mean_squared_error"],
                    loss_weights=[1 / 200, 199 / 200], clipnorm=1.0)
        rng = np.random.default_rng(0)
        y = [torch.as_tensor(rng.normal(size=(args.graphs, 1)).astype(np.float32)).cuda(),
             torch.as_tensor(rng.normal(size=(int(b["node_splits"][-1]), 3)).astype(np.float32) * 0.01).cuda()]
        res["train_step_ms"] = timed(lambda: efm.train_on_batch(inputs, y), args.steps, args.warmup)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
