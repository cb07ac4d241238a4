"""Engine calls per forward and time per replayed forward of the default RGCN and GNNFilm (depth 3, 20 relations) on 128
QM9-sized graphs, fused route against the layer sequence, alternating the two routes in one process."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gcnn_keras_amd import _ffi, synth  # noqa: E402
from gcnn_keras_amd.literature import GNNFilm, RGCN  # noqa: E402
from gcnn_keras_amd.ragged import RaggedTensor  # noqa: E402

ROUNDS, REPLAYS = 7, 400


def main():
    torch.cuda.set_device(0)
    b = synth.relational_batch(128, min_atoms=9, max_atoms=29)
    print("batch: %d nodes, %d edges" % (b["node_splits"][-1], b["edge_splits"][-1]), flush=True)
    rag = RaggedTensor.from_numpy
    for kind, mod in (("RGCN", RGCN), ("GNNFilm", GNNFilm)):
        # the default softmax over one unit is the constant 1: a linear output lets the two routes be compared
        model = mod.make_model(output_mlp={"use_bias": True, "units": 1, "activation": "linear"})
        model.set_weights(list(synth.relational_params(model).values()))
        x = [rag(b["node_number"].astype(np.float32), b["node_splits"]), rag(b["edge_indices"], b["edge_splits"])]
        if kind == "RGCN":
            x.append(rag(b["edge_weights"], b["edge_splits"]))
        x.append(rag(b["edge_relations"], b["edge_splits"]))
        times = {True: [], False: []}
        launches, outs = {}, {}
        with torch.no_grad():
            for fused in (True, False):
                model.use_fused_relational = fused
                model.auto_graph = False
                model(x)
                count = _ffi.launch_count()
                outs[fused] = model(x).cpu().numpy()
                launches[fused] = _ffi.launch_count() - count
                model.auto_graph = True
            for _ in range(ROUNDS):
                for fused in (True, False):
                    model.use_fused_relational = fused      # drops the other route's graph: capture again
                    for _ in range(20):
                        model(x)
                    assert model.last_route == "graph"
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(REPLAYS):
                        model(x)
                    torch.cuda.synchronize()
                    times[fused].append((time.perf_counter() - t0) / REPLAYS * 1e6)
        diff = float(np.max(np.abs(outs[True] - outs[False])))
        for fused in (True, False):
            t = np.array(times[fused])
            print("%s %s: %d engine calls per forward; replayed forward median %.1f us (min %.1f, max %.1f over %d x %d)"
                  % (kind, "fused" if fused else "layer sequence", launches[fused], float(np.median(t)), t.min(), t.max(),
                     ROUNDS, REPLAYS), flush=True)
        print("%s: routes differ by %.2e (output scale %.3g)" % (kind, diff, float(np.max(np.abs(outs[False])))), flush=True)


if __name__ == "__main__":
    main()
