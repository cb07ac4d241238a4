"""Regenerates tests/golden/scaler_cases.npz and tests/golden/scaler_reference.json.  Run ONLY in the build container
(it imports scikit-learn, which no test, smoke run or benchmark does):

    python -B tests/golden/make_scaler_fixtures.py

Source (data only; no reference source text is stored): the reference's scaler module cannot be imported here (its
package pulls in TensorFlow), so this script calls ``sklearn.linear_model.Ridge`` and NumPy in the op order of
kgcnn/data/transform/scaler/mol.py:55-74 (fit), :87-97 (predict) and kgcnn/data/transform/scaler/force.py:164-222
(transform / inverse transform) and stores the inputs and the float64 results.  scikit-learn 1.7 returns a 1-D ``coef_``
and prediction for a single target column; they are stored in the (n_states, n_species) / (n_samples, n_states) shapes
that the reference's arithmetic assumes (and that the scikit-learn versions the fork ran with return).

Cases (key prefix):

a   the five molecules of the reference's docstring (force.py:32-36), one state;
b   ``synth.qm9_like_batch(40, seed=3)``, species {1, 6, 7, 8, 9}; energies = per-element offsets -13.6 ... -2715 eV plus
    N(0, 0.3), float64; ragged float32 forces;
c   ``synth.md17_like_batch(6, seed=5)``: one composition repeated, the normal matrix is singular up to alpha;
d   12 molecules, two states, ``sample_weight``, ``fit_intercept=True``, forces (N, 3, 2);
e   the shapes a kernel can get wrong: 257 molecules (one more than the normal-equation chunk of 256) with an empty
    graph and a 130-atom graph among them;
e1  one molecule, ``standardize_scale=False``;
ex  a transform set with a species (16) that the fit of case ``e`` did not see (it contributes 0, mol.py:92-94).

Keys per case ``<c>``: ``numbers_<c>`` (flat int64) and ``splits_<c>``, ``energy_<c>`` (G, S) float64, ``force_<c>`` flat
float32, ``weight_<c>`` where used, ``counts_<c>`` (G, 95) int32, ``mask_<c>`` (95) bool, ``selection_<c>``,
``coef_<c>`` (S, K), ``intercept_<c>`` (S), ``scale_<c>`` (S), ``offset_<c>`` (G, S), ``energy_t_<c>`` / ``force_t_<c>``
(the transform), ``energy_inv_<c>`` (the inverse transform of ``energy_t_<c>``), ``cond_<c>`` (condition number of the
normal matrix).  ``ex`` holds numbers, energies, forces and the results under the weights of ``e``.

``scaler_reference.json`` is case ``b`` in the layout the fork's ``save`` writes (mol.py:242-252).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
MAX_Z = 95
ELEMENT_ENERGY = {1: -13.6, 6: -1029.9, 7: -1485.3, 8: -2042.6, 9: -2715.3, 16: -10832.3}


def count_matrix(numbers):
    """mol.py:55-67 / :87-96 without the selection: (G, 95) counts."""
    rows = []
    for x in numbers:
        unique_per_mol, num_unique = np.unique(x, return_counts=True)
        array_atoms = np.zeros(MAX_Z)
        array_atoms[unique_per_mol] = num_unique
        rows.append(array_atoms)
    return np.array(rows).reshape(len(numbers), MAX_Z)


def fit(numbers, energy, weight=None, alpha=1e-9, fit_intercept=False, standardize_scale=True):
    from sklearn.linear_model import Ridge
    counts = count_matrix(numbers)
    all_unique = np.unique(np.concatenate([np.unique(x) for x in numbers], axis=0)).astype(np.int64)
    atom_mask = np.zeros(MAX_Z, dtype="bool")
    atom_mask[all_unique] = True
    total_number = counts[:, atom_mask]
    ridge = Ridge(alpha=alpha, fit_intercept=fit_intercept)
    ridge.fit(total_number, energy, sample_weight=weight)
    diff = energy - ridge.predict(total_number).reshape(energy.shape)
    scale = np.std(diff, axis=0) if standardize_scale else np.ones(diff.shape[1:], dtype="float")
    w = np.ones(len(numbers)) if weight is None else np.asarray(weight, dtype=np.float64)
    x = total_number - (np.average(total_number, axis=0, weights=w) if fit_intercept else 0.0)
    normal = (x * w[:, None]).T @ x + alpha * np.eye(x.shape[1])
    return {"ridge": ridge, "mask": atom_mask, "selection": all_unique, "scale": scale, "counts": counts,
            "standardize_scale": standardize_scale, "cond": np.linalg.cond(normal)}


def apply(model, numbers, energy, force_rows):
    """force.py:164-171 and :207-215 (the copy branches)."""
    total_number = count_matrix(numbers)[:, model["mask"]]
    offset = model["ridge"].predict(total_number).reshape(np.shape(energy))
    scale = np.expand_dims(model["scale"], axis=0)
    y = np.array(energy) - offset
    if model["standardize_scale"]:
        y = y / scale
        force = [np.array(f, dtype=np.float64) / scale for f in force_rows]
    else:
        force = [np.array(f, dtype=np.float64) for f in force_rows]
    y_inv = y * scale if model["standardize_scale"] else np.array(y)
    force_inv = [f * scale for f in force] if model["standardize_scale"] else [np.array(f) for f in force]
    y_inv = y_inv + offset
    return offset, y, force, y_inv, force_inv


def energies(rng, numbers, states=1):
    base = np.array([sum(ELEMENT_ENERGY[int(z)] for z in x) for x in numbers], dtype=np.float64)
    cols = [base * (1.0 + 0.01 * s) + rng.normal(0.0, 0.3, size=len(numbers)) for s in range(states)]
    return np.stack(cols, axis=1)


def forces(rng, numbers, states=1):
    shape = (3,) if states == 1 else (3, states)
    return [rng.normal(0.0, 1.5, size=(len(x),) + shape).astype(np.float32) for x in numbers]


def flat(rows, dtype, inner=()):
    rows = [np.asarray(r, dtype=dtype).reshape((len(r),) + inner) for r in rows]
    return np.concatenate(rows, axis=0) if rows else np.zeros((0,) + inner, dtype)


def store(out, tag, numbers, energy, force_rows, model, weight=None):
    offset, y, f, y_inv, f_inv = apply(model, numbers, energy, force_rows)
    inner = tuple(force_rows[0].shape[1:])
    out["numbers_" + tag] = flat(numbers, np.int64)
    out["splits_" + tag] = np.concatenate([[0], np.cumsum([len(x) for x in numbers])]).astype(np.int64)
    out["energy_" + tag] = energy
    out["force_" + tag] = flat(force_rows, np.float32, inner)
    if weight is not None:
        out["weight_" + tag] = np.asarray(weight, dtype=np.float64)
    out["counts_" + tag] = count_matrix(numbers).astype(np.int32)
    out["mask_" + tag] = model["mask"]
    out["selection_" + tag] = model["selection"]
    out["coef_" + tag] = np.asarray(model["ridge"].coef_, dtype=np.float64).reshape(energy.shape[1], -1)
    out["intercept_" + tag] = np.broadcast_to(np.asarray(model["ridge"].intercept_, dtype=np.float64),
                                              (energy.shape[1],)).copy()
    out["scale_" + tag] = model["scale"]
    out["offset_" + tag] = offset
    out["energy_t_" + tag] = y
    if tag != "e":                           # case e's 1 200 force rows are float32(force) / scale: not stored (size)
        out["force_t_" + tag] = flat(f, np.float64, inner)
    out["energy_inv_" + tag] = y_inv         # the inverse of the forces is force_t * scale: not stored (fixture size)
    out["cond_" + tag] = np.float64(model["cond"])


def split_rows(b):
    ns = b["node_splits"]
    return [b["node_number"][ns[i]:ns[i + 1]].astype(np.int64) for i in range(len(ns) - 1)]


def main():
    sys.dont_write_bytecode = True
    from gcnn_keras_amd import synth
    rng = np.random.default_rng(2024)
    out = {}

    mol_num = [np.array([6, 1, 1, 1, 1]), np.array([7, 1, 1, 1]), np.array([6, 6, 1, 1, 1, 1]), np.array([6, 6, 1, 1]),
               np.array([6, 6, 1, 1, 1, 1, 1, 1])]
    energy = rng.random(5).reshape((5, 1))
    force = [rng.random(len(m) * 3).reshape((len(m), 3)).astype(np.float32) for m in mol_num]
    store(out, "a", mol_num, energy, force, fit(mol_num, energy))

    numbers = split_rows(synth.qm9_like_batch(40, seed=3))
    energy_b, force_b = energies(rng, numbers), forces(rng, numbers)
    model_b = fit(numbers, energy_b)
    store(out, "b", numbers, energy_b, force_b, model_b)

    numbers = split_rows(synth.md17_like_batch(num_graphs=6, seed=5))
    energy = energies(rng, numbers)
    store(out, "c", numbers, energy, forces(rng, numbers), fit(numbers, energy))

    numbers = split_rows(synth.qm9_like_nodes(12, seed=9))
    energy = energies(rng, numbers, states=2)
    weight = rng.uniform(0.5, 2.0, size=12)
    store(out, "d", numbers, energy, forces(rng, numbers, states=2),
          fit(numbers, energy, weight=weight, fit_intercept=True), weight=weight)

    species = np.array([1, 6, 7, 8])
    numbers = [rng.choice(species, size=int(rng.integers(1, 4)), p=[.5, .3, .1, .1]) for _ in range(257)]
    numbers[17] = np.zeros(0, dtype=np.int64)                                  # a graph with no atoms
    numbers[200] = rng.choice(species, size=130, p=[.5, .3, .1, .1])           # more atoms than a wave has lanes
    energy = energies(rng, numbers)
    model_e = fit(numbers, energy)
    store(out, "e", numbers, energy, forces(rng, numbers), model_e)

    numbers = [np.array([8, 1, 1])]
    energy = energies(rng, numbers)
    store(out, "e1", numbers, energy, forces(rng, numbers), fit(numbers, energy, standardize_scale=False))

    numbers = [np.array([6, 1, 1, 16, 1]), np.array([8, 1, 1]), np.array([16, 16])]
    store(out, "ex", numbers, energies(rng, numbers), forces(rng, numbers), model_e)

    path = os.path.join(HERE, "scaler_cases.npz")
    np.savez_compressed(path, **out)

    ridge = model_b["ridge"]
    config = dict(ridge.get_params())
    config.update({"standardize_scale": True, "standardize_coordinates": False, "energy": "energy", "force": "force",
                   "atomic_number": "atomic_number", "sample_weight": None})
    weights = {"scale_": model_b["scale"].tolist(), "_fit_atom_selection": model_b["selection"].tolist(),
               "_fit_atom_selection_mask": model_b["mask"].tolist()}
    for name in ["n_features_in_", "coef_", "intercept_", "n_iter_", "feature_names_in_"]:
        if hasattr(ridge, name):
            weights[name] = np.array(getattr(ridge, name)).tolist()
    weights["coef_"] = np.asarray(ridge.coef_).reshape(energy_b.shape[1], -1).tolist()
    info = {"class_name": "EnergyForceExtensiveLabelScaler", "module_name": "kgcnn.data.transform.scaler.force",
            "config": config, "weights": weights}
    jpath = os.path.join(HERE, "scaler_reference.json")
    with open(jpath, "w") as f:
        json.dump(info, f)
    print("arrays:", len(out), "npz bytes:", os.path.getsize(path), "json bytes:", os.path.getsize(jpath))
    print("cond:", {k[5:]: float(v) for k, v in out.items() if k.startswith("cond_")})


if __name__ == "__main__":
    main()
