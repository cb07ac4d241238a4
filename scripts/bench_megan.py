"""MEGAN (units [32, 32, 32], two importance channels, edge features) on ``synth.megan_batch(num_graphs=128)`` - the
``qm9_like_batch`` graphs with 12 node and 6 edge features - on one MI355X.

    python scripts/bench_megan.py

Prints ONE JSON line: the forward replayed from a captured HIP graph, the eager forward and one ``train_on_batch`` step
(regression with the explanation co-training step), each on the fused readout (csrc/mp_megan.hip) and on the baseline
``use_fused_readout = False`` - the route that issues only entry points the parent commit has, the attention block as it
is - and the engine calls per forward and per step of both.  The routes alternate in one process after warm-up; the times
are device events around ``--repeats`` calls, the median of ``--rounds`` rounds.  A parity configuration, not the headline
line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from gcnn_keras_amd import _ffi, synth
from gcnn_keras_amd.literature import MEGAN
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
    b = synth.megan_batch(num_graphs=args.graphs)
    n, m = int(b["node_splits"][-1]), int(b["edge_splits"][-1])
    x = [RaggedTensor.from_numpy(b["node_attributes"], b["node_splits"]),
         RaggedTensor.from_numpy(b["edge_attributes"], b["edge_splits"]),
         RaggedTensor.from_numpy(b["edge_indices"], b["edge_splits"])]
    y = torch.from_numpy(np.random.default_rng(3).uniform(-1.0, 1.0, size=(args.graphs, 1)).astype(np.float32)).cuda()
    inputs = [{"shape": (None, 12), "name": "node_attributes", "dtype": "float32", "ragged": True},
              {"shape": (None, 6), "name": "edge_attributes", "dtype": "float32", "ragged": True},
              {"shape": (None, 2), "name": "edge_indices", "dtype": "int64", "ragged": True}]
    kwargs = dict(units=[32, 32, 32], importance_channels=2, use_edge_features=True, return_importances=False,
                  regression_limits=(-1.0, 1.0), regression_reference=0.0, importance_factor=1.0, sparsity_factor=0.1)

    def make(fused, weights=None):
        mdl = MEGAN.make_model(inputs=inputs, **kwargs)
        mdl.set_weights(weights if weights is not None else list(synth.megan_params(mdl).values()))
        mdl.use_fused_readout = fused
        return mdl

    base = make(True)
    assert base.fused_readout and base.use_fused_attention
    weights = base.get_weights()
    out = {"workload": "MEGAN units [32, 32, 32], K=2, edge features on megan_batch(%d): N=%d, M=%d" % (args.graphs, n, m),
           "nodes": n, "edges": m}
    # one model per route, so that alternating the routes does not recapture in every round
    replay, eager, train = {}, {}, {}
    for fused in (True, False):
        tag = "fused_readout" if fused else "baseline"
        replay[fused], eager[fused], train[fused] = make(fused, weights), make(fused, weights), make(fused, weights)
        eager[fused].auto_graph = False
        train[fused].compile(optimizer=torch.optim.SGD(train[fused].trainable_weights, lr=1e-4), loss="mean_squared_error")
        with torch.no_grad():
            for _ in range(3):
                replay[fused](x)
            assert replay[fused].last_route == "graph", replay[fused].last_route
            eager[fused](x)
            count = _ffi.launch_count()
            eager[fused](x)
            out["calls_per_forward_" + tag] = _ffi.launch_count() - count
        assert eager[fused].last_readout_route == ("fused" if fused else "layers")
        train[fused].train_on_batch(x, y)
        count = _ffi.launch_count()
        train[fused].train_on_batch(x, y)
        out["calls_per_step_" + tag] = _ffi.launch_count() - count
    times = {}
    for _ in range(args.rounds):
        for fused in (True, False):
            with torch.no_grad():
                replay[fused](x)
                times.setdefault((fused, "forward_replayed_ms"), []).append(event_ms(lambda: replay[fused](x), args.repeats))
                eager[fused](x)
                times.setdefault((fused, "forward_eager_ms"), []).append(event_ms(lambda: eager[fused](x), args.repeats))
            train[fused].train_on_batch(x, y)
            times.setdefault((fused, "train_step_ms"), []).append(
                event_ms(lambda: train[fused].train_on_batch(x, y), args.repeats))
    for (fused, what), v in times.items():
        out["%s_%s" % (what, "fused_readout" if fused else "baseline")] = float(np.median(v))
    with torch.no_grad():
        out["max_abs_difference_between_routes"] = float((replay[True](x) - replay[False](x)).abs().max())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
