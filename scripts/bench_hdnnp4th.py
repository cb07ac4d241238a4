"""HDNNP4th at the fork's configuration (force_hdnnp4th.py:41-71, 151-246; charge_hdnnp4th.py): 128
alanine-dipeptide-shaped molecules with total charges and the electrostatic potential of MM point charges.

Times (median of HIP events, per call): the ``"charge+qm_energy"`` forward (eager layer path and the replayed
auto-graph), energy + forces on the inference tape with the esp chain (``EnergyForceModel(energy_output=1, esp_input=5,
esp_grad_input=6, is_physical_force=False)``), one ``train_on_batch`` step of the charge model (``output_embedding=
"charge"``, MSE on ragged charges, Adam, clipnorm 1.0) and one of the total-energy model (``"graph"``).  Prints one JSON
line.  A kernel breakdown: ``rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_hdnnp4th.py --only forward``."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gcnn_keras_amd import synth                        # noqa: E402
from gcnn_keras_amd.literature import HDNNP4th          # noqa: E402
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


def model(embedding):
    m = HDNNP4th.make_model_behler(**synth.hdnnp4th_model_kwargs(output_embedding=embedding))
    m.set_weights(list(synth.hdnnp4th_params().values())[:len(m.weights)])
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["all", "forward", "force", "train"], default="all")
    args = ap.parse_args()
    b = synth.hdnnp4th_batch(num_graphs=args.graphs, seed=4567)
    ns = b["node_splits"]
    inputs = [RaggedTensor.from_numpy(b["node_number"], ns), RaggedTensor.from_numpy(b["node_coordinates"], ns),
              RaggedTensor.from_numpy(b["edge_indices"], b["edge_splits"]),
              RaggedTensor.from_numpy(b["angle_indices"], b["angle_splits"]),
              torch.as_tensor(b["total_charge"]).cuda(), RaggedTensor.from_numpy(b["esp"], ns),
              RaggedTensor.from_numpy(b["esp_grad"], ns)]
    res = {"graphs": args.graphs, "atoms": int(ns[-1]), "edges": int(b["edge_splits"][-1]),
           "triplets": int(b["angle_splits"][-1]), "steps": args.steps}
    m = model("charge+qm_energy")
    if args.only in ("all", "forward"):
        m.auto_graph = False
        res["forward_eager_ms"] = timed(lambda: m(inputs), args.steps, args.warmup)
        m.auto_graph = True
        res["forward_replayed_ms"] = timed(lambda: m(inputs), args.steps, args.warmup)
    if args.only in ("all", "force"):
        efm = EnergyForceModel(model_energy=m, energy_output=1, esp_input=5, esp_grad_input=6, output_as_dict=False,
                               output_squeeze_states=True, is_physical_force=False)
        res["energy_force_ms"] = timed(lambda: efm(inputs), args.steps, args.warmup)
    if args.only in ("all", "train"):
        rng = np.random.default_rng(0)
        mc = model("charge")
        mc.compile(optimizer="adam", loss="mean_squared_error", clipnorm=1.0)
        q_t = RaggedTensor.from_numpy((rng.normal(size=(int(ns[-1]), 1)) * 0.3).astype(np.float32), ns)
        res["charge_train_step_ms"] = timed(lambda: mc.train_on_batch(inputs, q_t), args.steps, args.warmup)
        me = model("graph")
        me.compile(optimizer="adam", loss="mean_squared_error", clipnorm=1.0)
        e_t = torch.as_tensor(rng.normal(size=(args.graphs, 1)).astype(np.float32)).cuda()
        res["energy_train_step_ms"] = timed(lambda: me.train_on_batch(inputs, e_t), args.steps, args.warmup)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
