"""Cost of one force-training step of the fork's SchNet (force_schnet.py:33-45, 163-205: embedding 128, depth 6,
Gauss(25, 5.0, 0.4), last_mlp [128, 64, 1]; energy MSE + force MSE weighted [1/200, 199/200], Adam, clipnorm 1.0) on
128 MD17-shaped molecules, beside the energy-only ``train_on_batch`` and the inference tape (energy + forces, layer path)
of the same batch.

    python scripts/bench_force_training.py [--graphs 128] [--steps 20] [--warmup 3] [--force-only]

Every figure is the median over ``--steps`` calls of HIP events recorded around one call on torch's stream, after
``--warmup`` calls.  Prints ONE JSON line (milliseconds).  ``--force-only`` runs the force-training steps alone (the
workload of a kernel trace)."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from gcnn_keras_amd import _ffi, synth
from gcnn_keras_amd.literature import Schnet
from gcnn_keras_amd.model.force import EnergyForceModel
from gcnn_keras_amd.ragged import RaggedTensor

FORK = dict(
    inputs=[{"shape": [None], "name": "node_number", "dtype": "int64", "ragged": True},
            {"shape": [None, 3], "name": "node_coordinates", "dtype": "float32", "ragged": True},
            {"shape": [None, 2], "name": "range_indices", "dtype": "int64", "ragged": True}],
    input_embedding={"node": {"input_dim": 95, "output_dim": 128}},
    interaction_args={"units": 128, "use_bias": True, "activation": "shifted_softplus", "cfconv_pool": "sum"},
    node_pooling_args={"pooling_method": "sum"}, depth=6,
    gauss_args={"bins": 25, "distance": 5, "offset": 0.0, "sigma": 0.4}, verbose=10,
    last_mlp={"use_bias": [True] * 3, "units": [128, 64, 1], "activation": ["shifted_softplus"] * 2 + ["linear"]},
    output_embedding="graph", output_to_tensor=True, use_output_mlp=False, output_mlp=None)


def median_ms(fn, steps, warmup):
    start, stop = ctypes.c_void_p(), ctypes.c_void_p()
    _ffi.call("mp_event_create", ctypes.byref(start))
    _ffi.call("mp_event_create", ctypes.byref(stop))
    try:
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(steps):
            _ffi.call("mp_event_record", start, _ffi.stream())
            fn()
            _ffi.call("mp_event_record", stop, _ffi.stream())
            torch.cuda.synchronize()
            ms = ctypes.c_float(0.0)
            _ffi.call("mp_event_elapsed_ms", start, stop, ctypes.byref(ms))
            times.append(ms.value)
        return float(np.median(times))
    finally:
        _ffi.call("mp_event_destroy", start)
        _ffi.call("mp_event_destroy", stop)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--force-only", action="store_true")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    b = synth.md17_like_batch(num_graphs=args.graphs, seed=2345)
    p = synth.schnet_params(seed=7, depth=6, emb_out=128, bins=25, last_units=(128, 64, 1), out_units=(),
                            random_bias=True)
    inputs = [RaggedTensor.from_numpy(b["node_number"].astype(np.int64), b["node_splits"]),
              RaggedTensor.from_numpy(b["node_coordinates"], b["node_splits"]),
              RaggedTensor.from_numpy(b["edge_indices"], b["edge_splits"])]
    n, m = int(b["node_splits"][-1]), int(b["edge_splits"][-1])
    rng = np.random.default_rng(1)
    e_t = rng.normal(size=(args.graphs, 1)).astype(np.float32)
    f_t = RaggedTensor.from_numpy(rng.normal(size=(n, 3)).astype(np.float32), b["node_splits"])

    energy = Schnet.make_model(**FORK)
    energy.set_weights(list(p.values()))
    efm = EnergyForceModel(model_energy=energy, coordinate_input=1, energy_output=0, output_as_dict=False,
                           output_to_tensor=True, output_squeeze_states=True, is_physical_force=False)
    efm.compile(optimizer="adam", loss=["mean_squared_error", "mean_squared_error"], loss_weights=[1 / 200, 199 / 200],
                clipnorm=1.0)
    t_force = median_ms(lambda: efm.train_on_batch(inputs, [e_t, f_t]), args.steps, args.warmup)
    if args.force_only:
        print(json.dumps({"workload": "fork SchNet force training step", "graphs": args.graphs, "nodes": n, "edges": m,
                          "train_on_batch_energy_force_ms": round(t_force, 3)}))
        return

    energy_only = Schnet.make_model(**FORK)
    energy_only.set_weights(list(p.values()))
    energy_only.compile(optimizer="adam", loss="mean_squared_error")
    t_energy = median_ms(lambda: energy_only.train_on_batch(inputs, e_t), args.steps, args.warmup)

    tape = EnergyForceModel(model_energy=energy_only, coordinate_input=1, energy_output=0, output_as_dict=False,
                            output_to_tensor=False, output_squeeze_states=True, is_physical_force=False)
    tape.fused = False
    t_tape = median_ms(lambda: tape(inputs), args.steps, args.warmup)

    print(json.dumps({"workload": "fork SchNet force training step", "device": torch.cuda.get_device_name(0),
                      "graphs": args.graphs, "nodes": n, "edges": m, "steps": args.steps, "warmup": args.warmup,
                      "train_on_batch_energy_force_ms": round(t_force, 3),
                      "train_on_batch_energy_only_ms": round(t_energy, 3),
                      "inference_tape_energy_force_ms": round(t_tape, 3),
                      "force_step_over_energy_step": round(t_force / t_energy, 2)}))


if __name__ == "__main__":
    main()
