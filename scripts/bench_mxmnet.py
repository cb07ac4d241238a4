"""MXMNet at the reference's width-128, depth-6 configuration (synth.MXMNET_MD17, the model section of
training/results/MD17Dataset/MXMNet_EnergyForceModel/*; the QM9 runs use the same sizes): 64 MD17-shaped molecules
(21 atoms, local edges within 3 A) or 128 QM9-shaped graphs (3 to 29 atoms, bond-like local edges within 2 A), the global
edges within 5 A.

Times (median of HIP events over --steps calls after --warmup calls), each alternated call by call between the fused
route and the reference's layer sequence on the same inputs: one ``MXMGlobalMP.propagate`` (``mp_mxm_edge_f32`` behind
two node-sized Dense launches against gather, concatenate, two Dense, multiply, PoolingLocalMessages, add), one
``MXMLocalMP`` with the edge messages alone, the triplet pools alone and both switched, the eager forward, energy +
forces through ``EnergyForceModel`` (the tape), and the forward replayed from the auto-graph on either route; beside
them the engine calls of one call on either route, and the forward and the force pass on the mix of routes the model
ships with (``model.use_fused_step = None``).  Prints one JSON line.  A kernel breakdown:
``rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_mxmnet.py --only forward``."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gcnn_keras_amd import _ffi, synth                                     # noqa: E402
from gcnn_keras_amd.literature import MXMNet                               # noqa: E402
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


def calls_of(fn):
    before = _ffi.launch_count()
    fn()
    return _ffi.launch_count() - before


def batch_of(config, graphs):
    if config == "md17":
        return synth.mxmnet_batch(num_graphs=graphs, local_distance=3.0)
    sizes = np.diff(synth.qm9_like_nodes(num_graphs=graphs)["node_splits"]).tolist()
    return synth.mxmnet_batch(sizes=sizes, seed=1234, sigma=1.6, local_distance=2.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=None, help="default: 64 (md17), 128 (qm9)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", choices=["md17", "qm9"], default="md17")
    ap.add_argument("--only", choices=["all", "forward", "force", "steps"], default="all")
    args = ap.parse_args()
    graphs = args.graphs or (64 if args.config == "md17" else 128)
    b = batch_of(args.config, graphs)
    rag = RaggedTensor.from_numpy
    inputs = [rag(b["node_number"], b["node_splits"]), rag(b["node_coordinates"], b["node_splits"]),
              rag(b["edge_weights"], b["edge_splits"]), rag(b["edge_indices"], b["edge_splits"]),
              rag(b["angle_indices_1"], b["angle_splits_1"]), rag(b["angle_indices_2"], b["angle_splits_2"]),
              rag(b["range_indices"], b["range_splits"])]
    res = {"config": args.config, "graphs": graphs, "atoms": int(b["node_splits"][-1]),
           "edges": int(b["edge_splits"][-1]), "range_edges": int(b["range_splits"][-1]),
           "triplets_1": int(b["angle_splits_1"][-1]), "triplets_2": int(b["angle_splits_2"][-1]),
           "steps": args.steps, "warmup": args.warmup}
    m = MXMNet.make_model(**synth.MXMNET_MD17)
    m.set_weights(list(synth.mxmnet_params(m).values()))
    glob, loc = m.global_blocks[0], m.local_blocks[0]
    width = glob.dim

    def forward(fused):
        m.use_fused_step = fused
        return m(inputs)

    def pair(key, fn, on, off):
        """``fn`` under the switch settings ``on`` and ``off``: alternated medians and the engine calls of one call."""
        def run(setting):
            setting()
            return fn()
        run(on), run(off)   # build the plans and their CSRs outside the timed calls
        res[key + "_fused_ms"], res[key + "_layers_ms"] = timed_pair(lambda: run(on), lambda: run(off), args.steps,
                                                                     args.warmup)
        res[key + "_fused_calls"], res[key + "_layers_calls"] = calls_of(lambda: run(on)), calls_of(lambda: run(off))

    with torch.no_grad():
        if args.only in ("all", "steps"):
            rng = np.random.default_rng(0)

            def values(like, cols):
                rows = int(like.values.shape[0])
                return like.with_values(torch.from_numpy(rng.normal(size=(rows, cols)).astype(np.float32)).cuda())

            h = values(inputs[1], width)
            rbf_g, rbf_l = values(inputs[6], width), values(inputs[3], width)
            sbf1, sbf2 = values(inputs[4], width), values(inputs[5], width)

            def set_global(flag):
                glob.use_fused_step = flag

            def set_local(edge, triplet):
                loc.use_fused_step, loc.use_fused_triplet = edge, triplet

            pair("propagate", lambda: glob.propagate(inputs[6], h, rbf_g),
                 lambda: set_global(True), lambda: set_global(False))
            local = lambda: loc([h, rbf_l, sbf1, sbf2, inputs[3], inputs[4], inputs[5]])   # noqa: E731
            pair("local_edge", local, lambda: set_local(True, False), lambda: set_local(False, False))
            pair("local_triplet", local, lambda: set_local(False, True), lambda: set_local(False, False))
            pair("local", local, lambda: set_local(True, True), lambda: set_local(False, False))
            m.use_fused_step = None
        if args.only in ("all", "forward"):
            m.auto_graph = False
            res["forward_fused_ms"], res["forward_layers_ms"] = timed_pair(
                lambda: forward(True), lambda: forward(False), args.steps, args.warmup)
            res["forward_fused_calls"] = calls_of(lambda: forward(True))
            res["forward_layers_calls"] = calls_of(lambda: forward(False))
            m.use_fused_step = None   # the mix the model ships with
            res["forward_shipped_ms"] = timed(lambda: m(inputs), args.steps, args.warmup)
            res["forward_shipped_calls"] = calls_of(lambda: m(inputs))
            m.auto_graph = True
            for fused, key in ((True, "forward_replayed_fused_ms"), (False, "forward_replayed_layers_ms"),
                               (None, "forward_replayed_shipped_ms")):
                m.use_fused_step = fused
                res[key] = timed(lambda: m(inputs), args.steps, args.warmup)
                res[key.replace("_ms", "_route")] = m.last_route
    if args.only in ("all", "force"):
        efm = EnergyForceModel(model_energy=m, coordinate_input=1, output_to_tensor=False, output_squeeze_states=True)

        def force(fused):
            m.use_fused_step = fused
            return efm(inputs)

        res["energy_force_fused_ms"], res["energy_force_layers_ms"] = timed_pair(
            lambda: force(True), lambda: force(False), args.steps, args.warmup)
        res["energy_force_fused_calls"] = calls_of(lambda: force(True))
        res["energy_force_layers_calls"] = calls_of(lambda: force(False))
        res["energy_force_shipped_ms"] = timed(lambda: force(None), args.steps, args.warmup)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
