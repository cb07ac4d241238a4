"""AttentiveFP on ``synth.cmpnn_batch(num_graphs=128)`` on one MI355X: ``model_default`` (embedding inputs, units 32) and
the paper's width (``units=200``, feature inputs: the heads are outside the served sizes there, the readout is served).

    python scripts/bench_attentivefp.py

Prints ONE JSON line: per configuration and route the engine calls per forward and the forward time, eager and replayed
from a captured HIP graph.  Routes: ``fused`` (every served layer on csrc/mp_attentivefp.hip / csrc/mp_gat.hip),
``layer_sequence`` (``model.use_fused_attentive = False``: the baseline, engine layers and kernels that exist unchanged at
the parent commit), ``heads_only`` and ``readout_only`` (one kind of layer fused), so that each fused route is judged on
its own.  The routes alternate in one process after warm-up; the times are device events around ``--repeats`` forwards, the
median of ``--rounds`` rounds.  A parity configuration, not the headline line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from gcnn_keras_amd import _ffi, synth
from gcnn_keras_amd.literature import AttentiveFP
from gcnn_keras_amd.ragged import RaggedTensor

ROUTES = {"fused": (True, True), "layer_sequence": (False, False), "heads_only": (True, False),
          "readout_only": (False, True)}


def event_ms(fn, repeats):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(repeats):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / repeats


def set_route(model, route):
    heads, readout = ROUTES[route]
    for lay in model.attention_heads:
        lay.use_fused_attentive = heads
    model.readout.use_fused_attentive = readout


def configurations(b):
    rag = RaggedTensor.from_numpy
    idx = rag(b["edge_indices"], b["edge_splits"])
    yield ("model_default", {},
           [rag(b["node_number"].astype(np.float32), b["node_splits"]),
            rag(b["edge_number"].astype(np.float32), b["edge_splits"]), idx])
    fn, fe = b["node_attributes"].shape[1], b["edge_attributes"].shape[1]
    spec = [{"shape": (None, fn), "name": "node_attributes", "dtype": "float32", "ragged": True},
            {"shape": (None, fe), "name": "edge_attributes", "dtype": "float32", "ragged": True},
            {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True}]
    yield ("units200_features", {"attention_args": {"units": 200}, "inputs": spec},
           [rag(b["node_attributes"], b["node_splits"]), rag(b["edge_attributes"], b["edge_splits"]), idx])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    b = synth.cmpnn_batch(num_graphs=args.graphs)
    n, m = int(b["node_splits"][-1]), int(b["edge_splits"][-1])
    out = {"workload": "AttentiveFP on cmpnn_batch(%d): N=%d, M=%d" % (args.graphs, n, m), "nodes": n, "edges": m}
    for name, kwargs, x in configurations(b):
        model = AttentiveFP.make_model(**kwargs)
        weights = list(synth.attentivefp_params(model).values())
        model.set_weights(weights)
        res = {"fused_attentive_blocks": model.fused_attentive_blocks}
        model.auto_graph = False
        for route in ROUTES:
            set_route(model, route)
            with torch.no_grad():
                model(x)
                count = _ffi.launch_count()
                model(x)
            res["launches_" + route] = _ffi.launch_count() - count
        # one model per route for the replay, so that alternating the routes does not recapture in every round
        replay = {}
        for route in ROUTES:
            mdl = AttentiveFP.make_model(**kwargs)
            mdl.set_weights(weights)
            set_route(mdl, route)
            with torch.no_grad():
                for _ in range(3):
                    mdl(x)
            res["replay_route_" + route] = mdl.last_route   # "graph", or "eager" where the capture failed
            replay[route] = mdl
        times = {}
        for _ in range(args.rounds):
            for route in ROUTES:
                set_route(model, route)
                with torch.no_grad():
                    model(x)                               # warm-up of this route after the switch
                    times.setdefault((route, "eager"), []).append(event_ms(lambda: model(x), args.repeats))
                    times.setdefault((route, "graph"), []).append(event_ms(lambda: replay[route](x), args.repeats))
        for (route, how), v in times.items():
            res["forward_ms_%s_%s" % (route, how)] = float(np.median(v))
        with torch.no_grad():
            res["max_abs_difference_between_routes"] = float((replay["fused"](x) - replay["layer_sequence"](x)).abs().max())
        out[name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
