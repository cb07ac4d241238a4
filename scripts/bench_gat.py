"""GAT / GATv2 ``model_default`` (embedding inputs, units 32, 5 heads, depth 3) on ``synth.qm9_like_batch(num_graphs=128)``
on one MI355X.

    python scripts/bench_gat.py

Prints ONE JSON line: per builder the forward time on the fused attention route (csrc/mp_gat.hip) and on the layer
sequence (``model.use_fused_attention = False``, the baseline on the same commit), each eager and replayed from a captured
HIP graph, and the engine calls per forward of both routes.  The two routes alternate in one process after warm-up; the
times are device events around ``--repeats`` forwards, the median of ``--rounds`` rounds.  A parity configuration, not the
headline line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from gcnn_keras_amd import _ffi, synth
from gcnn_keras_amd.literature import GAT, GATv2
from gcnn_keras_amd.ragged import RaggedTensor


def event_ms(fn, repeats):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(repeats):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / repeats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    b = synth.qm9_like_batch(num_graphs=args.graphs)
    n, m = int(b["node_splits"][-1]), int(b["edge_splits"][-1])
    edge_type = np.random.default_rng(5).integers(0, 5, size=m).astype(np.float32)
    x = [RaggedTensor.from_numpy(b["node_number"], b["node_splits"]), RaggedTensor.from_numpy(edge_type, b["edge_splits"]),
         RaggedTensor.from_numpy(b["edge_indices"], b["edge_splits"])]
    out = {"workload": "GAT / GATv2 model_default on qm9_like_batch(%d): N=%d, M=%d" % (args.graphs, n, m),
           "nodes": n, "edges": m}
    for name, builder in (("GAT", GAT), ("GATv2", GATv2)):
        model = builder.make_model()
        assert model.fused_attention_blocks == [True] * 3

        def forward(fused, graph):
            model.use_fused_attention = fused          # a change of route drops the captured graphs
            model.auto_graph = graph
            with torch.no_grad():
                return model(x)

        res, times = {}, {}
        for fused in (True, False):
            forward(fused, False)
            count = _ffi.launch_count()
            forward(fused, False)
            res["launches_" + ("fused" if fused else "layer_sequence")] = _ffi.launch_count() - count
        # one model per route for the replay, so that alternating the routes does not recapture in every round
        replay = {}
        for fused in (True, False):
            mdl = builder.make_model()
            mdl.set_weights(model.get_weights())
            mdl.use_fused_attention = fused
            with torch.no_grad():
                for _ in range(3):
                    mdl(x)
            assert mdl.last_route == "graph", mdl.last_route
            replay[fused] = mdl
        model.auto_graph = False
        for _ in range(args.rounds):
            for fused in (True, False):
                model.use_fused_attention = fused
                with torch.no_grad():
                    model(x)                           # warm-up of this route after the switch
                    times.setdefault((fused, "eager"), []).append(event_ms(lambda: model(x), args.repeats))
                    times.setdefault((fused, "graph"), []).append(event_ms(lambda: replay[fused](x), args.repeats))
        for (fused, how), v in times.items():
            res["forward_ms_%s_%s" % ("fused" if fused else "layer_sequence", how)] = float(np.median(v))
        same = float((replay[True](x) - replay[False](x)).abs().max())
        res["max_abs_difference_between_routes"] = same
        out[name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
