"""MD inference step (kgcnn/moldyn/base.py:106-165, one molecule, energy + forces): latency of
``MolDynamicsModelPredictor.__call__`` on one 21-atom MD17-shaped molecule with a PaiNN ``EnergyForceModel``, eager and
with ``use_graph=True``; ``--profile`` adds a cProfile table of the host side of the replayed step.  ``--scaler`` also
times the replayed step with an ``ExtensiveEnergyForceScalerPostprocessor`` behind the model, in host form
(``graph_postprocessors``: NumPy per molecule) and in device form (``tensor_postprocessors``: one launch in front of the
read-back), alternated with the plain step in rounds so that all three see the same machine state.

    python scripts/bench_moldyn.py [--profile] [--scaler] [steps]
"""
import cProfile
import json
import os
import pstats
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch

from gcnn_keras_amd import synth
from gcnn_keras_amd.moldyn import MolDynamicsModelPredictor
from test_gpu_moldyn import ITEMS, _graphs, _painn_ef


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    steps = int(args[0]) if args else 300
    model = _painn_ef()
    b = synth.md17_like_batch(num_graphs=1, seed=6)
    outs = {"energy": "energy", "forces": "force"}
    eager = MolDynamicsModelPredictor(model=model, model_inputs=ITEMS, model_outputs=outs)
    fast = MolDynamicsModelPredictor(model=model, model_inputs=ITEMS, model_outputs=outs, use_graph=True)
    rng = np.random.default_rng(0)
    xyz = b["node_coordinates"].copy()

    def run(pred, n):
        x = xyz
        for _ in range(n):
            x = x + rng.normal(scale=0.001, size=x.shape).astype(np.float32)
            pred(_graphs(b, x))

    run(eager, 5), run(fast, 5)
    torch.cuda.synchronize()
    t0 = time.perf_counter(); run(eager, 30); torch.cuda.synchronize(); t_eager = (time.perf_counter() - t0) / 30
    t0 = time.perf_counter(); run(fast, steps); torch.cuda.synchronize(); t_fast = (time.perf_counter() - t0) / steps
    print(json.dumps({"workload": "MD step: PaiNN energy + forces, one 21-atom molecule, N=%d, M=%d"
                                  % (int(b["node_splits"][-1]), int(b["edge_splits"][-1])),
                      "step_ms_eager": t_eager * 1e3, "step_ms_graph_replay": t_fast * 1e3,
                      "graph_captures": fast.graph_captures}))
    if "--scaler" in sys.argv:
        from gcnn_keras_amd.data.transform.scaler import EnergyForceExtensiveLabelScaler
        from gcnn_keras_amd.graph.postprocessor import ExtensiveEnergyForceScalerPostprocessor
        scaler = EnergyForceExtensiveLabelScaler()      # aspirin offsets; the weights' values do not change the timing
        scaler.set_weights({"scale_": [0.17], "_fit_atom_selection": [1, 6, 8], "coef_": [[-13.6, -1029.9, -2042.6]],
                            "_fit_atom_selection_mask": [z in (1, 6, 8) for z in range(95)], "intercept_": 0.0,
                            "n_features_in_": 3})
        post = ExtensiveEnergyForceScalerPostprocessor(scaler)
        preds = {"plain": fast,
                 "host": MolDynamicsModelPredictor(model=model, model_inputs=ITEMS, model_outputs=outs, use_graph=True,
                                                   graph_postprocessors=[post]),
                 "device": MolDynamicsModelPredictor(model=model, model_inputs=ITEMS, model_outputs=outs, use_graph=True,
                                                     tensor_postprocessors=[post])}
        for pred in preds.values():
            run(pred, 5)
        rounds, per = 5, max(steps // 5, 1)
        times = {k: [] for k in preds}
        for _ in range(rounds):
            for k, pred in preds.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter(); run(pred, per); torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) / per * 1e3)
        print(json.dumps({"workload": "MD step with the scaler postprocessor (graph replay), %d rounds x %d steps"
                                      % (rounds, per),
                          "step_ms_median": {k: float(np.median(v)) for k, v in times.items()},
                          "step_ms_min": {k: float(np.min(v)) for k, v in times.items()},
                          "step_ms_max": {k: float(np.max(v)) for k, v in times.items()}}))
    if "--profile" in sys.argv:
        pr = cProfile.Profile()
        pr.enable(); run(fast, steps); pr.disable()
        st = pstats.Stats(pr, stream=sys.stdout).sort_stats("cumulative")
        st.print_stats(45)


if __name__ == "__main__":
    main()
