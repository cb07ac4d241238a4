"""Label scaler on a resident data set: ``EnergyForceExtensiveLabelScaler.fit`` + ``transform`` of QM9-shaped molecules
whose numbers, float64 energies and float32 forces are already on the device (the state ``fit`` of a model finds them
in), against the reference's host path (kgcnn/data/transform/scaler/mol.py:55-74 + force.py:164-171: ``np.unique`` per
molecule, ``sklearn.linear_model.Ridge``, NumPy) where scikit-learn is installed.

    python scripts/bench_scaler.py [molecules]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from gcnn_keras_amd import synth
from gcnn_keras_amd.data.transform.scaler import EnergyForceExtensiveLabelScaler
from gcnn_keras_amd.ragged import RaggedTensor

ELEMENT_ENERGY = {1: -13.6, 6: -1029.9, 7: -1485.3, 8: -2042.6, 9: -2715.3}


def host_reference(rows, energy, force_rows):
    from sklearn.linear_model import Ridge
    unique_number = [np.unique(x, return_counts=True) for x in rows]
    all_unique = np.unique(np.concatenate([x[0] for x in unique_number], axis=0))
    atom_mask = np.zeros(95, dtype="bool")
    atom_mask[all_unique] = True
    total_number = []
    for unique_per_mol, num_unique in unique_number:
        array_atoms = np.zeros(95)
        array_atoms[unique_per_mol] = num_unique
        total_number.append(array_atoms[atom_mask])
    total_number = np.array(total_number)
    ridge = Ridge(alpha=1e-9, fit_intercept=False).fit(total_number, energy)
    offset = ridge.predict(total_number).reshape(energy.shape)
    scale = np.std(energy - offset, axis=0)
    return (energy - offset) / scale[None, :], [f / scale[None, :] for f in force_rows], scale


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    G = int(args[0]) if args else 100000
    b = synth.qm9_like_nodes(G, seed=77)
    ns = b["node_splits"]
    z = b["node_number"].astype(np.int64)
    rng = np.random.default_rng(5)
    per_atom = np.vectorize(ELEMENT_ENERGY.get, otypes=[np.float64])(z)
    energy = (np.add.reduceat(per_atom, ns[:-1]) + rng.normal(0.0, 0.3, size=G)).reshape(G, 1)
    force = rng.normal(0.0, 1.5, size=(len(z), 3)).astype(np.float32)
    numbers = RaggedTensor.from_numpy(b["node_number"], ns)
    e_dev = torch.from_numpy(energy).cuda()
    f_dev = RaggedTensor.from_numpy(force, ns)

    def device_once():
        scaler = EnergyForceExtensiveLabelScaler()
        scaler.fit(y=(e_dev, f_dev), X=numbers)
        t0 = time.perf_counter()
        out = scaler.transform(y=(e_dev, f_dev), X=numbers)
        torch.cuda.synchronize()
        return scaler, out, time.perf_counter() - t0

    device_once()
    fit_ms, all_ms, xform_ms = [], [], []
    for _ in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scaler, out, t_x = device_once()
        all_ms.append((time.perf_counter() - t0) * 1e3)
        xform_ms.append(t_x * 1e3)
        fit_ms.append(all_ms[-1] - xform_ms[-1])
    result = {"workload": "scaler fit + transform, %d QM9-shaped molecules (%d atoms) resident on the device" % (G, len(z)),
              "device_fit_ms_median": float(np.median(fit_ms)), "device_transform_ms_median": float(np.median(xform_ms)),
              "device_fit_transform_ms": {"median": float(np.median(all_ms)), "min": float(np.min(all_ms)),
                                          "max": float(np.max(all_ms))}}
    try:
        import sklearn  # noqa: F401
        rows = [z[ns[i]:ns[i + 1]] for i in range(G)]
        f_rows = [force[ns[i]:ns[i + 1]] for i in range(G)]
        host_ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            y_h, _, scale_h = host_reference(rows, energy, f_rows)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        result["host_sklearn_fit_transform_ms"] = {"median": float(np.median(host_ms)), "min": float(np.min(host_ms)),
                                                   "max": float(np.max(host_ms))}
        result["scale_rel_diff"] = float(abs(scaler.scale_[0] - scale_h[0]) / scale_h[0])
        result["max_abs_label_diff"] = float(np.max(np.abs(out[0].cpu().numpy() - y_h)))
    except ImportError:
        result["host_sklearn_fit_transform_ms"] = "scikit-learn is not installed here: not measured"
    print(json.dumps(result))


if __name__ == "__main__":
    main()
