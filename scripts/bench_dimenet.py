"""DimeNet++ at the reference's MD17 force-field configuration (synth.DIMENET_MD17, the model section of
training/results/MD17Dataset/DimeNetPP_EnergyForceModel/*): 64 MD17-shaped molecules (BASELINE config 3, 5 A cutoff,
angle pairs of get_angle_indices with "jk" pairing).

Times (median of HIP events over --steps calls after --warmup calls): the forward (eager layer path and the replayed
auto-graph), energy + forces through ``EnergyForceModel`` (the tape), and the triplet step of one interaction block -
the fused ``mp_dimenet_triplet_f32`` against the reference's layer sequence (GatherNodesOutgoing, two Dense,
LazyMultiply, PoolingLocalEdges), alternated call by call on the same inputs.  Prints one JSON line.  A kernel
breakdown: ``rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_dimenet.py --only forward``."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gcnn_keras_amd import synth                                           # noqa: E402
from gcnn_keras_amd.layers.conv.dimenet_conv import DimNetInteractionPPBlock  # noqa: E402
from gcnn_keras_amd.literature import DimeNetPP                            # noqa: E402
from gcnn_keras_amd.model.force import EnergyForceModel                    # noqa: E402
from gcnn_keras_amd.ragged import RaggedTensor                             # noqa: E402


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return float(np.median([_event_ms(fn) for _ in range(steps)]))


def timed_pair(fn_a, fn_b, steps, warmup):
    """Medians of two calls alternated a, b, a, b, ... (same clocks, same caches for both)."""
    for _ in range(warmup):
        fn_a()
        fn_b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(steps):
        ta.append(_event_ms(fn_a))
        tb.append(_event_ms(fn_b))
    return float(np.median(ta)), float(np.median(tb))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["all", "forward", "force", "triplet"], default="all")
    args = ap.parse_args()
    b = synth.dimenet_batch(num_graphs=args.graphs)
    inputs = [RaggedTensor.from_numpy(b["node_number"], b["node_splits"]),
              RaggedTensor.from_numpy(b["node_coordinates"], b["node_splits"]),
              RaggedTensor.from_numpy(b["edge_indices"], b["edge_splits"]),
              RaggedTensor.from_numpy(b["angle_indices"], b["angle_splits"])]
    res = {"graphs": args.graphs, "atoms": int(b["node_splits"][-1]), "edges": int(b["edge_splits"][-1]),
           "triplets": int(b["angle_splits"][-1]), "steps": args.steps, "warmup": args.warmup}
    m = DimeNetPP.make_model(**synth.DIMENET_MD17)
    m.set_weights(list(synth.dimenet_params(m).values()))
    with torch.no_grad():
        if args.only in ("all", "forward"):
            m.auto_graph = False
            res["forward_eager_ms"] = timed(lambda: m(inputs), args.steps, args.warmup)
            m.auto_graph = True
            res["forward_replayed_ms"] = timed(lambda: m(inputs), args.steps, args.warmup)
        if args.only in ("all", "triplet"):
            block = [layer for layer in m.layers if isinstance(layer, DimNetInteractionPPBlock)][0]
            rng = np.random.default_rng(0)
            e = res["edges"]
            ref = inputs[2].with_values(torch.zeros((e, 1), device="cuda"))
            xdown = ref.with_values(torch.from_numpy(rng.normal(size=(e, 64)).astype(np.float32)).cuda())
            rbf = ref.with_values(torch.from_numpy(rng.normal(size=(e, 128)).astype(np.float32)).cuda())
            sbf = inputs[3].with_values(torch.from_numpy(rng.normal(size=(res["triplets"], 42)).astype(np.float32))
                                        .cuda())

            def step(fused):
                block.use_fused_triplet = fused
                return block.triplet_step(xdown, rbf, sbf, inputs[3])

            step(True), step(False)   # build the plan and its CSRs outside the timed calls
            res["triplet_fused_ms"], res["triplet_layer_sequence_ms"] = timed_pair(
                lambda: step(True), lambda: step(False), args.steps, args.warmup)
            block.use_fused_triplet = True
            res["triplet_speedup"] = res["triplet_layer_sequence_ms"] / res["triplet_fused_ms"]
    if args.only in ("all", "force"):
        efm = EnergyForceModel(model_energy=m, coordinate_input=1, output_to_tensor=False, output_squeeze_states=True)
        res["energy_force_ms"] = timed(lambda: efm(inputs), args.steps, args.warmup)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
