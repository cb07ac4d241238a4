"""EGNN at the reference's MD17 force-field configuration (synth.EGNN_MD17, the model section of
training/results/MD17Dataset/EGNN_EnergyForceModel/*): 64 MD17-shaped molecules, fully connected (10 A cutoff).

Times (median of HIP events over --steps calls after --warmup calls): the edge step of one block - the fused
``mp_egnn_edge_f32`` (node-side Dense + one kernel) against the reference's layer sequence (position encoding, gather,
concatenate, two Dense, attention Dense, multiply, PoolingLocalEdges) - the whole forward and energy + forces through
``EnergyForceModel`` (the tape), each alternated call by call between ``use_fused_edge`` True and False on the same
inputs, and the forward replayed from the auto-graph.  Prints one JSON line.  A kernel breakdown:
``rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_egnn.py --only forward [--layers]``."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gcnn_keras_amd import synth                                           # noqa: E402
from gcnn_keras_amd.layers.geom import EuclideanNorm, NodePosition         # noqa: E402
from gcnn_keras_amd.layers.modules import LazySubtract                     # noqa: E402
from gcnn_keras_amd.layers.pooling import PoolingLocalEdges                # noqa: E402
from gcnn_keras_amd.literature import EGNN                                 # noqa: E402
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
    ap.add_argument("--config", choices=["md17", "qm9"], default="md17")
    ap.add_argument("--only", choices=["all", "forward", "force", "edge"], default="all")
    ap.add_argument("--layers", action="store_true", help="with --only forward: time the layer sequence alone")
    args = ap.parse_args()
    b = synth.egnn_batch(num_graphs=args.graphs)
    inputs = [RaggedTensor.from_numpy(b["node_attributes"], b["node_splits"]),
              RaggedTensor.from_numpy(b["node_coordinates"], b["node_splits"]),
              RaggedTensor.from_numpy(b["edge_indices"], b["edge_splits"])]
    res = {"config": args.config, "graphs": args.graphs, "atoms": int(b["node_splits"][-1]),
           "edges": int(b["edge_splits"][-1]), "steps": args.steps, "warmup": args.warmup}
    m = EGNN.make_model(**(synth.EGNN_MD17 if args.config == "md17" else synth.EGNN_QM9))
    m.set_weights(list(synth.egnn_params(m).values()))

    def forward(fused):
        m.use_fused_edge = fused
        return m(inputs)

    with torch.no_grad():
        if args.only in ("all", "edge"):
            rng = np.random.default_rng(0)
            h = inputs[0].with_values(torch.from_numpy(rng.normal(size=(res["atoms"], 128)).astype(np.float32)).cuda())
            p1, p2 = NodePosition()([inputs[1], inputs[2]])
            x = EuclideanNorm(axis=2, keepdims=True, square_norm=True)(LazySubtract()([p1, p2]))
            pool = PoolingLocalEdges(pooling_method="sum")

            def step(fused):
                m.use_fused_edge = fused
                m_ij, m_i = m.edge_step(0, h, x, None, inputs[2])
                return m_i if m_i is not None else pool([h, m_ij, inputs[2]])

            step(True), step(False)   # build the plan and its CSRs outside the timed calls
            res["edge_fused_ms"], res["edge_layer_sequence_ms"] = timed_pair(
                lambda: step(True), lambda: step(False), args.steps, args.warmup)
            res["edge_speedup"] = res["edge_layer_sequence_ms"] / res["edge_fused_ms"]
        if args.only in ("all", "forward"):
            m.auto_graph = False
            if args.only == "forward":
                res["forward_%s_ms" % ("layers" if args.layers else "fused")] = timed(
                    lambda: forward(not args.layers), args.steps, args.warmup)
            else:
                res["forward_fused_ms"], res["forward_layers_ms"] = timed_pair(
                    lambda: forward(True), lambda: forward(False), args.steps, args.warmup)
            m.auto_graph, m.use_fused_edge = True, not args.layers
            res["forward_replayed_ms"] = timed(lambda: m(inputs), args.steps, args.warmup)
            m.use_fused_edge = True
    if args.only in ("all", "force"):
        efm = EnergyForceModel(model_energy=m, coordinate_input=1, output_to_tensor=False, output_squeeze_states=True)

        def force(fused):
            m.use_fused_edge = fused
            return efm(inputs)

        res["energy_force_fused_ms"], res["energy_force_layers_ms"] = timed_pair(
            lambda: force(True), lambda: force(False), args.steps, args.warmup)
        m.use_fused_edge = True
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
