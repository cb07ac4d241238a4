"""On-GPU batching against the host packer, on QM9-shaped graphs with the three inputs of ``bench.py run_stream``
(node numbers, coordinates, edge indices), timed with HIP events on the current stream:

1. one ``take_batch`` of 128 shuffled graphs out of the resident data set, next to ``BatchPacker.pack(...).wait()`` of the
   same graphs from the host lists;
2. one shuffled SchNet epoch through ``Model.fit``, against the same batches (``batch_ids``) packed by the host packer and
   fed to ``train_on_batch``.

Prints one JSON line.  ``python scripts/bench_fit.py [--graphs 1024] [--batch 128] [--repeats 50] [--epochs 5]``"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gcnn_keras_amd import synth  # noqa: E402
from gcnn_keras_amd.data.batching import batch_ids, take_batch  # noqa: E402
from gcnn_keras_amd.data.packer import BatchPacker  # noqa: E402
from gcnn_keras_amd.literature import Schnet  # noqa: E402
from gcnn_keras_amd.ragged import RaggedTensor  # noqa: E402

ITEMS = [{"name": "node_number", "ragged": True, "dtype": "float32"},
         {"name": "node_coordinates", "ragged": True, "dtype": "float32"},
         {"name": "edge_indices", "ragged": True, "dtype": "int64"}]


def graph_list(b):
    ns, es = b["node_splits"], b["edge_splits"]
    return [{"node_number": b["node_number"][ns[g]:ns[g + 1]], "node_coordinates": b["node_coordinates"][ns[g]:ns[g + 1]],
             "edge_indices": b["edge_indices"][es[g]:es[g + 1]]} for g in range(len(ns) - 1)]


def timed(fn, repeats):
    """Milliseconds per call of ``fn`` between two HIP events on the current stream (median of ``repeats``)."""
    ms = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        ms.append(start.elapsed_time(stop))
    return float(np.median(ms)), float(np.min(ms))


def model_and_target(graphs):
    model = Schnet.make_model(depth=3)
    model.set_weights(list(synth.schnet_params(seed=7, random_bias=True).values()))
    model.compile(optimizer="sgd", loss="mean_absolute_error")
    return model, np.random.default_rng(4).normal(size=(graphs, 1)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--epochs", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fit.py measures on the GPU only"
    b = synth.qm9_like_batch(num_graphs=args.graphs, seed=1234)
    graphs = graph_list(b)
    x = [RaggedTensor.from_numpy(b["node_number"], b["node_splits"]),
         RaggedTensor.from_numpy(b["node_coordinates"], b["node_splits"]),
         RaggedTensor.from_numpy(b["edge_indices"], b["edge_splits"])]
    ids = batch_ids(args.graphs, args.batch, shuffle=True, seed=3, epoch=0)[0]
    ids_dev = torch.from_numpy(ids).cuda()
    packer = BatchPacker(ITEMS, index_item="edge_indices", node_item="node_number", slots=4)
    picked = [graphs[i] for i in ids]
    for _ in range(5):
        take_batch(x, ids_dev, ids)
        packer.pack(picked).wait()
    torch.cuda.synchronize()
    take_ms = timed(lambda: take_batch(x, ids_dev, ids), args.repeats)
    pack_ms = timed(lambda: packer.pack(picked).wait(), args.repeats)

    def fit_epoch(model, y, epoch):
        model.fit(x, y, batch_size=args.batch, epochs=epoch + 1, initial_epoch=epoch, shuffle=True, seed=3)

    def packed_epoch(model, target, epoch):
        for batch in batch_ids(args.graphs, args.batch, shuffle=True, seed=3, epoch=epoch):
            pb = packer.pack([graphs[i] for i in batch]).wait()
            model.train_on_batch([pb["node_number"], pb["node_coordinates"], pb["edge_indices"]], target[batch])

    fit_model, target = model_and_target(args.graphs)
    y = torch.from_numpy(target).cuda()
    pack_model, _ = model_and_target(args.graphs)
    fit_epoch(fit_model, y, 0)
    packed_epoch(pack_model, target, 0)
    torch.cuda.synchronize()
    fit_ms, packed_ms = [], []
    for epoch in range(1, args.epochs + 1):       # alternate the two, same batches per epoch
        fit_ms.append(timed(lambda: fit_epoch(fit_model, y, epoch), 1)[0])
        packed_ms.append(timed(lambda: packed_epoch(pack_model, target, epoch), 1)[0])
    same = all(torch.equal(s, t) for s, t in zip(fit_model.trainable_weights, pack_model.trainable_weights))
    print(json.dumps({
        "device": torch.cuda.get_device_name(0), "graphs": args.graphs, "batch": args.batch,
        "nodes_per_batch": int(sum(len(g["node_number"]) for g in picked)),
        "edges_per_batch": int(sum(len(g["edge_indices"]) for g in picked)),
        "take_batch_ms_median_min": take_ms, "host_packer_ms_median_min": pack_ms,
        "fit_epoch_ms": fit_ms, "packed_epoch_ms": packed_ms, "steps_per_epoch": -(-args.graphs // args.batch),
        "weights_equal_after": bool(same)}))


if __name__ == "__main__":
    main()
