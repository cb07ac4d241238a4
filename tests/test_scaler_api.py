"""Host side of the extensive energy / force label scaler (gcnn_keras_amd/data/transform/scaler, mirror of
kgcnn/data/transform/scaler/{mol,force}.py) and of its MD postprocessor: constructor guards, config and JSON round trips,
the reference-layout ``scaler.json``, the NumPy host form of the postprocessor.  No GPU (there is no CPU ``fit``)."""
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = np.load(os.path.join(GOLDEN, "scaler_cases.npz"))
REFERENCE_JSON = os.path.join(GOLDEN, "scaler_reference.json")


def _rows(tag, key, inner=()):
    s = CASES["splits_" + tag]
    v = CASES[key + "_" + tag]
    return [v[s[i]:s[i + 1]] for i in range(len(s) - 1)]


def test_constructor_guards():
    from gcnn_keras_amd.data.transform.scaler import EnergyForceExtensiveLabelScaler, ExtensiveMolecularLabelScaler
    with pytest.raises(NotImplementedError):
        EnergyForceExtensiveLabelScaler(standardize_coordinates=True)
    for cls in (EnergyForceExtensiveLabelScaler, ExtensiveMolecularLabelScaler):
        with pytest.raises(NotImplementedError):
            cls(positive=True)
        for solver in ("svd", "lsqr", "sparse_cg", "sag", "saga", "lbfgs"):
            with pytest.raises(NotImplementedError):
                cls(solver=solver)
        with pytest.raises(TypeError):
            cls(no_such_ridge_parameter=1)
        assert cls(solver="cholesky").get_config()["solver"] == "cholesky"
        assert cls().get_config()["alpha"] == 1e-9 and cls().get_config()["fit_intercept"] is False


def test_config_round_trip_and_reference_keys():
    from gcnn_keras_amd.data.transform.scaler import EnergyForceExtensiveLabelScaler, ExtensiveMolecularLabelScaler
    reference = json.load(open(REFERENCE_JSON))
    scaler = EnergyForceExtensiveLabelScaler(alpha=1e-6, fit_intercept=True, standardize_scale=False, energy="e",
                                             force="f", atomic_number="z", sample_weight="w", tol=1e-3, max_iter=7)
    config = scaler.get_config()
    assert set(config) == set(reference["config"])            # the fork's keys: Ridge.get_params() + the scaler's own
    assert (config["alpha"], config["fit_intercept"], config["standardize_scale"]) == (1e-6, True, False)
    assert (config["energy"], config["force"], config["atomic_number"], config["sample_weight"]) == ("e", "f", "z", "w")
    assert (config["tol"], config["max_iter"], config["copy_X"], config["solver"]) == (1e-3, 7, True, "auto")
    assert EnergyForceExtensiveLabelScaler().set_config(config).get_config() == config
    assert EnergyForceExtensiveLabelScaler().get_config() == reference["config"]
    with pytest.raises(NotImplementedError):
        EnergyForceExtensiveLabelScaler().set_config(dict(config, standardize_coordinates=True))
    with pytest.raises(NotImplementedError):
        EnergyForceExtensiveLabelScaler().set_config(dict(config, solver="svd"))
    label = ExtensiveMolecularLabelScaler(y="labels", atomic_number="z", fit_intercept=True)
    config = label.get_config()
    assert config["y"] == "labels" and config["atomic_number"] == "z" and config["sample_weight"] is None
    assert ExtensiveMolecularLabelScaler().set_config(config).get_config() == config


def test_reference_json_loads():
    from gcnn_keras_amd.data.transform.scaler import EnergyForceExtensiveLabelScaler
    scaler = EnergyForceExtensiveLabelScaler().load(REFERENCE_JSON)
    assert np.array_equal(scaler.scale_, CASES["scale_b"])
    assert np.array_equal(scaler.ridge.coef_, CASES["coef_b"])
    assert np.array_equal(scaler._fit_atom_selection, [1, 6, 7, 8, 9])
    assert np.array_equal(scaler._fit_atom_selection_mask, CASES["mask_b"]) and scaler._fit_atom_selection_mask.dtype == bool
    assert scaler.ridge.n_features_in_ == 5 and float(scaler.ridge.intercept_) == 0.0
    assert np.array_equal(scaler.get_scaling(), CASES["scale_b"][None, :])
    assert scaler.get_config() == json.load(open(REFERENCE_JSON))["config"]


def test_save_then_load_reproduces_weights_and_config(tmp_path):
    from gcnn_keras_amd.data.transform.scaler import EnergyForceExtensiveLabelScaler, ExtensiveMolecularLabelScaler
    scaler = EnergyForceExtensiveLabelScaler(fit_intercept=True, alpha=1e-7, energy="E")
    scaler.set_weights({"scale_": CASES["scale_d"].tolist(), "_fit_atom_selection": CASES["selection_d"].tolist(),
                        "_fit_atom_selection_mask": CASES["mask_d"].tolist(), "coef_": CASES["coef_d"].tolist(),
                        "intercept_": CASES["intercept_d"].tolist(), "n_features_in_": int(len(CASES["selection_d"]))})
    path = str(tmp_path / "scaler.json")
    scaler.save(path)
    info = json.load(open(path))
    assert list(info) == ["class_name", "module_name", "config", "weights"]
    assert info["class_name"] == "EnergyForceExtensiveLabelScaler"
    assert set(info["weights"]) == {"scale_", "_fit_atom_selection", "_fit_atom_selection_mask", "coef_", "intercept_",
                                    "n_features_in_"}
    loaded = EnergyForceExtensiveLabelScaler().load(path)
    assert loaded.get_config() == scaler.get_config() and loaded.get_config()["energy"] == "E"
    ours, theirs = scaler.get_weights(), loaded.get_weights()
    assert set(ours) == set(theirs)
    for key in ours:
        assert np.array_equal(np.asarray(ours[key]), np.asarray(theirs[key])), key
    assert np.array_equal(loaded.ridge.coef_, CASES["coef_d"]) and np.array_equal(loaded.ridge.intercept_, CASES["intercept_d"])
    # the energies-only scaler shares the layout
    label = ExtensiveMolecularLabelScaler(y="labels")
    label.set_weights(scaler.get_weights())
    label.save(str(tmp_path / "label.json"))
    again = ExtensiveMolecularLabelScaler().load(str(tmp_path / "label.json"))
    assert again.get_config() == label.get_config() and again.get_weights() == label.get_weights()


def test_host_postprocessor_returns_the_golden_inverse_transform(capsys):
    from gcnn_keras_amd.data.transform.scaler import EnergyForceExtensiveLabelScaler
    from gcnn_keras_amd.graph.postprocessor import ExtensiveEnergyForceScalerPostprocessor
    scaler = EnergyForceExtensiveLabelScaler().load(REFERENCE_JSON)
    post = ExtensiveEnergyForceScalerPostprocessor(scaler)
    numbers, force_t, force = _rows("b", "numbers"), _rows("b", "force_t"), _rows("b", "force")
    bar = 1e-12 * float(np.max(np.abs(CASES["energy_b"])))
    for i in (0, 7, 39):
        out = post(graph={"energy": CASES["energy_t_b"][i], "forces": force_t[i]},
                   pre_graph={"node_number": numbers[i].astype(np.float32)})
        assert set(out) == {"energy", "forces"} and out["energy"].dtype == np.float64 and out["energy"].shape == (1,)
        assert np.max(np.abs(out["energy"] - CASES["energy_inv_b"][i])) <= bar
        # force_t * scale in float64 gives back the float32 force it was made from, to float64 rounding
        assert out["forces"].shape == force[i].shape
        assert np.max(np.abs(out["forces"] - force[i].astype(np.float64))) <= 4 * np.finfo(np.float64).eps * 10.0
    assert capsys.readouterr().out == ""
    post(graph={"energy": np.zeros(1), "forces": np.zeros((2, 3))}, pre_graph={"node_number": np.array([1, 16])})
    assert "unknown atom species" in capsys.readouterr().out
    with pytest.raises(TypeError):
        ExtensiveEnergyForceScalerPostprocessor({"class_name": "EnergyForceExtensiveLabelScaler"})


def test_unfitted_and_unequal_inputs_raise_value_error():
    from gcnn_keras_amd.data.transform.scaler import EnergyForceExtensiveLabelScaler, ExtensiveMolecularLabelScaler
    numbers, force = _rows("a", "numbers"), _rows("a", "force")
    energy = CASES["energy_a"]
    with pytest.raises(ValueError):
        EnergyForceExtensiveLabelScaler().inverse_transform(y=(energy, force), X=numbers)
    with pytest.raises(ValueError):
        EnergyForceExtensiveLabelScaler().transform(y=(energy, force), X=numbers)
    with pytest.raises(ValueError):
        ExtensiveMolecularLabelScaler().inverse_transform(y=energy, X=numbers)
    with pytest.raises(ValueError):
        EnergyForceExtensiveLabelScaler().fit(y=(energy, force), X=numbers[:4])          # 5 energies, 4 molecules
    with pytest.raises(ValueError):
        ExtensiveMolecularLabelScaler().fit(y=energy[:3], X=numbers)
    with pytest.raises(ValueError):
        ExtensiveMolecularLabelScaler().fit(X=numbers)                                     # no labels
    with pytest.raises(ValueError):
        EnergyForceExtensiveLabelScaler().fit(X=numbers)
    fitted = EnergyForceExtensiveLabelScaler().load(REFERENCE_JSON)
    with pytest.raises(ValueError):
        fitted.transform(y=(energy, force[:4]), X=numbers)
    with pytest.raises(ValueError):
        fitted.inverse_transform(y=(energy, force), X=numbers[:2])
    with pytest.raises(ValueError):
        fitted.transform(y=energy[:2], force=force[:3], atomic_number=numbers)             # the deprecated form's rule
