"""Extensive energy / force label scaler on the GPU (csrc/mp_scaler.hip, gcnn_keras_amd/data/transform/scaler) against
tests/golden/scaler_cases.npz: ``sklearn.linear_model.Ridge`` + NumPy in the reference's op order, float64
(tests/golden/make_scaler_fixtures.py).

Bars.  ``E`` = max |energy| of the case, ``eps32`` = 2^-23.
* ``coef_``, ``intercept_``, ``scale_`` of the well-conditioned cases (a, b, d, e: condition number of the normal matrix
  <= 686, asserted below): 1e-8 relative, element by element.  cond x eps64 = 1.5e-13 leaves five orders.
* FP64 offsets and FP64 inverse-transformed energies of those cases: 1e-12 x E.  LAPACK and a NumPy Cholesky differ by
  2e-16 relative at E = 4e4; the bar leaves four orders for the reduction order.
* float32 outputs: one float32 ulp of the golden value plus that bar divided by ``scale_``.  "One ulp" of x is taken as
  eps32 |x| throughout (the spacing of float32 at x lies in (eps32 |x| / 2, eps32 |x|]).
* the singular cases (c: one composition repeated, condition 1e12; e1: one molecule, 5e9): coefficients are NOT compared
  (two FP64 solvers differ by 55 % there, the null-space component is arbitrary); offsets, ``scale_`` and transformed values
  of the fitted set are held to 1e-9 x E.
* round trip: forces come back to one float32 ulp (two roundings of 2^-24 each).  Energies come back to 1e-12 x E through
  float64 transformed energies (``dtype=torch.float64``); through the default float32 labels the round trip cannot be
  better than half a float32 ulp of the transformed value times ``scale_`` (2.6e-8 at E = 2.4e4 in case b), and that
  default path is held to exactly this bound on top of the 1e-12 x E.
"""
import os

import numpy as np
import pytest
import torch

from gcnn_keras_amd import _ffi, synth

pytestmark = pytest.mark.gpu

CASES = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scaler_cases.npz"))
EPS32 = float(np.finfo(np.float32).eps)
CONFIG = {"a": {}, "b": {}, "c": {}, "d": {"fit_intercept": True}, "e": {}, "e1": {"standardize_scale": False}}
NUMBER_DTYPES = {"int64": np.int64, "int32": np.int32, "float32": np.float32}


def _ragged(values, splits):
    from gcnn_keras_amd.ragged import RaggedTensor
    return RaggedTensor.from_numpy(values, splits)


def _rows(values, splits):
    return [values[splits[i]:splits[i + 1]] for i in range(len(splits) - 1)]


def _case(tag, number_dtype=np.int64):
    """Device form of a case: ragged numbers, (G, S) float64 energies, ragged float32 forces, sample weights or None."""
    s = CASES["splits_" + tag]
    numbers = _ragged(CASES["numbers_" + tag].astype(number_dtype), s)
    energy = torch.from_numpy(CASES["energy_" + tag]).cuda()
    force = _ragged(CASES["force_" + tag], s)
    weight = CASES["weight_" + tag] if "weight_" + tag in CASES else None
    return numbers, energy, force, weight


def _fit(tag, number_dtype=np.int64):
    from gcnn_keras_amd.data.transform.scaler import EnergyForceExtensiveLabelScaler
    numbers, energy, force, weight = _case(tag, number_dtype)
    scaler = EnergyForceExtensiveLabelScaler(**CONFIG[tag])
    scaler.fit(y=(energy, force), X=numbers, sample_weight=weight)
    return scaler, numbers, energy, force


def _weights(scaler):
    w = scaler.get_weights()
    S = len(w["scale_"])
    return (np.asarray(w["coef_"], np.float64).reshape(S, -1), np.broadcast_to(np.asarray(w["intercept_"], np.float64), (S,)),
            np.asarray(w["scale_"], np.float64))


def _species_count(values, splits):
    """``mp_scaler_species_count`` alone: counts (G, 95), mask (95), selection (96), flag word."""
    G = len(splits) - 1
    z = torch.from_numpy(np.ascontiguousarray(values)).cuda()
    sp = torch.from_numpy(np.ascontiguousarray(splits, dtype=np.int64)).cuda()
    counts = torch.full((G, 95), -7, dtype=torch.int32, device="cuda")
    mask = torch.full((95,), -7, dtype=torch.int32, device="cuda")
    sel = torch.full((96,), -7, dtype=torch.int32, device="cuda")
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    kind = {np.dtype(np.float32): _ffi.MP_DT_F32, np.dtype(np.int32): _ffi.MP_DT_I32, np.dtype(np.int64): _ffi.MP_DT_I64}
    _ffi.call("mp_scaler_species_count", _ffi.ptr(z), kind[values.dtype], _ffi.ptr(sp), G, len(values), _ffi.ptr(counts),
              _ffi.ptr(mask), _ffi.ptr(sel), _ffi.ptr(flags), _ffi.stream())
    return counts.cpu().numpy(), mask.cpu().numpy(), sel.cpu().numpy(), int(flags.item())


# --------------------------------------------------------------------------------------------------------- counts and mask
@pytest.mark.parametrize("dtype", sorted(NUMBER_DTYPES))
@pytest.mark.parametrize("tag", ["a", "b", "e"])
def test_counts_and_mask_equal_the_golden_bit_for_bit(tag, dtype):
    values = CASES["numbers_" + tag].astype(NUMBER_DTYPES[dtype])
    counts, mask, sel, flags = _species_count(values, CASES["splits_" + tag])
    assert counts.dtype == np.int32 and np.array_equal(counts, CASES["counts_" + tag])
    assert np.array_equal(mask.astype(bool), CASES["mask_" + tag]) and set(np.unique(mask)) <= {0, 1}
    K = int(sel[95])
    assert np.array_equal(sel[:K], CASES["selection_" + tag]) and np.all(sel[K:95] == -1)
    assert flags == 0


@pytest.mark.parametrize("dtype", sorted(NUMBER_DTYPES))
def test_out_of_range_number_sets_the_flag_and_changes_nothing_else(dtype):
    rows = _rows(CASES["numbers_a"], CASES["splits_a"])
    bad = [95, -3, 200, 2 ** 31 + 6 if dtype == "int64" else 1000]
    rows = [np.concatenate([rows[0], bad[:2]]), rows[1], np.concatenate([bad[2:], rows[2]]), rows[3], rows[4]]
    values = np.concatenate(rows).astype(NUMBER_DTYPES[dtype])
    if dtype == "float32":
        values[len(rows[0]) - 1] = np.nan                       # a NaN is out of range as well
    splits = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    counts, mask, sel, flags = _species_count(values, splits)
    assert flags == _ffi.MP_FLAG_OOB
    assert np.array_equal(counts, CASES["counts_a"]) and np.array_equal(mask.astype(bool), CASES["mask_a"])
    assert int(sel[95]) == len(CASES["selection_a"])


def test_float_numbers_are_cast_as_keras_casts_them():
    values = np.array([1.0, 6.9, 7.2, 0.5, -0.5, 94.99], dtype=np.float32)     # truncation: 1 6 7 0 0 94
    counts, _, _, flags = _species_count(values, np.array([0, 6]))
    want = np.zeros(95, np.int32)
    for k in (1, 6, 7, 0, 0, 94):
        want[k] += 1
    assert np.array_equal(counts[0], want) and flags == 0


# ------------------------------------------------------------------------------------------------------------ fit + apply
def _check_transforms(scaler, tag, numbers, energy, force, bar):
    """Offsets, forward float32 outputs and FP64 inverse energies of the fitted set against the golden, at ``bar``."""
    scale = CASES["scale_" + tag]
    offset = scaler._predict(numbers).cpu().numpy()
    err_offset = float(np.max(np.abs(offset - CASES["offset_" + tag])))
    e_t, f_t = scaler.transform(y=(energy, force), X=numbers)
    assert e_t.dtype == torch.float32 and f_t.values.dtype == torch.float32 and f_t.row_splits is force.row_splits
    assert tuple(e_t.shape) == tuple(energy.shape) and tuple(f_t.values.shape) == tuple(force.values.shape)
    gold_e = CASES["energy_t_" + tag]
    err_e = np.abs(e_t.cpu().numpy().astype(np.float64) - gold_e.astype(np.float32).astype(np.float64))
    bar_e = EPS32 * np.abs(gold_e) + bar / scale
    if "force_t_" + tag in CASES:
        gold_f = CASES["force_t_" + tag]
    else:
        gold_f = CASES["force_" + tag].astype(np.float64) / scale
    err_f = np.abs(f_t.values.cpu().numpy().astype(np.float64) - gold_f.astype(np.float32).astype(np.float64))
    bar_f = EPS32 * np.abs(gold_f) + bar / scale
    gold_t = torch.from_numpy(gold_e).cuda()
    e_inv, f_inv = scaler.inverse_transform(y=(gold_t, f_t), X=numbers)
    assert e_inv.dtype == torch.float64 and f_inv.values.dtype == torch.float32
    err_inv = float(np.max(np.abs(e_inv.cpu().numpy() - CASES["energy_inv_" + tag])))
    print("case %s: offset err %.3g, inverse energy err %.3g (bar %.3g); float32 energy err/bar %.3g, force err/bar %.3g"
          % (tag, err_offset, err_inv, bar, float(np.max(err_e / bar_e)), float(np.max(err_f / np.maximum(bar_f, 1e-300)))))
    assert err_offset <= bar and err_inv <= bar
    assert np.all(err_e <= bar_e) and np.all(err_f <= bar_f)
    return err_offset


@pytest.mark.parametrize("tag", ["a", "b", "d", "e"])
def test_fit_and_transform_of_the_well_conditioned_cases(tag):
    assert float(CASES["cond_" + tag]) <= 687.0 and abs(float(CASES["cond_b"]) - 686.0) < 0.1
    scaler, numbers, energy, force = _fit(tag)
    coef, intercept, scale = _weights(scaler)
    w = scaler.get_weights()
    assert np.array_equal(w["_fit_atom_selection"], CASES["selection_" + tag])
    assert np.array_equal(w["_fit_atom_selection_mask"], CASES["mask_" + tag])
    assert w["n_features_in_"] == len(CASES["selection_" + tag]) and scaler.check_flags() == 0
    assert (w["intercept_"] == 0.0) if not CONFIG[tag].get("fit_intercept") else (len(w["intercept_"]) == scale.size)
    for name, got, ref in (("coef_", coef, CASES["coef_" + tag]), ("intercept_", intercept, CASES["intercept_" + tag]),
                           ("scale_", scale, CASES["scale_" + tag])):
        assert got.shape == ref.shape, name
        rel = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)
        print("case %s %s: worst relative error %.3g" % (tag, name, float(np.max(np.where(ref == 0, np.abs(got), rel)))))
        assert np.all(np.abs(got - ref) <= 1e-8 * np.abs(ref)), name
    E = float(np.max(np.abs(CASES["energy_" + tag])))
    _check_transforms(scaler, tag, numbers, energy, force, 1e-12 * E)
    assert np.array_equal(scaler.get_scaling(), scale[None, :])


@pytest.mark.parametrize("tag", ["c", "e1"])
def test_singular_normal_matrix_offsets_scale_and_transforms(tag):
    assert float(CASES["cond_" + tag]) > 1e9
    scaler, numbers, energy, force = _fit(tag)
    _, _, scale = _weights(scaler)
    E = float(np.max(np.abs(CASES["energy_" + tag])))
    if tag == "e1":
        assert np.array_equal(scale, np.ones(1))                       # standardize_scale=False
    else:
        assert np.all(np.abs(scale - CASES["scale_" + tag]) <= 1e-9 * E)
    err = _check_transforms(scaler, tag, numbers, energy, force, 1e-9 * E)
    print("case %s: offsets off the golden by %.3g = %.3g x max|E|" % (tag, err, err / E))


def test_unknown_species_contributes_zero_and_raises_the_flag(capsys):
    scaler, _, _, _ = _fit("e")
    numbers, energy, force, _ = _case("ex")
    E = float(np.max(np.abs(CASES["energy_e"])))
    offset = scaler._predict(numbers).cpu().numpy()
    assert np.max(np.abs(offset - CASES["offset_ex"])) <= 1e-12 * E and offset[2, 0] == 0.0
    e_t, f_t = scaler.transform(y=(energy, force), X=numbers)
    assert scaler.check_flags() == _ffi.MP_FLAG_UNKNOWN_SPECIES
    bar = EPS32 * np.abs(CASES["energy_t_ex"]) + 1e-12 * E / CASES["scale_e"]
    assert np.all(np.abs(e_t.cpu().numpy() - CASES["energy_t_ex"].astype(np.float32)) <= bar)
    assert capsys.readouterr().out == ""                              # the tensor form reads nothing back and prints nothing
    s = CASES["splits_ex"]
    scaler.transform(y=(CASES["energy_ex"], _rows(CASES["force_ex"], s)), X=_rows(CASES["numbers_ex"], s))
    assert "unknown atom species" in capsys.readouterr().out          # the list form prints the reference's warning


# ---------------------------------------------------------------------------------------------- round trip and determinism
@pytest.mark.parametrize("tag", ["b", "d"])
def test_round_trip(tag):
    scaler, numbers, energy, force = _fit(tag)
    E = float(np.max(np.abs(CASES["energy_" + tag])))
    ref_e, ref_f = CASES["energy_" + tag], CASES["force_" + tag].astype(np.float64)
    e64, f_t = scaler.transform(y=(energy, force), X=numbers, dtype=torch.float64)
    back_e, back_f = scaler.inverse_transform(y=(e64, f_t), X=numbers)
    assert back_e.dtype == torch.float64
    err = float(np.max(np.abs(back_e.cpu().numpy() - ref_e)))
    err_f = np.abs(back_f.values.cpu().numpy().astype(np.float64) - ref_f)
    print("case %s: FP64 round trip %.3g (bar %.3g); forces worst %.3g ulp" % (tag, err, 1e-12 * E,
                                                                          float(np.max(err_f / (EPS32 * np.abs(ref_f))))))
    assert err <= 1e-12 * E
    assert np.all(err_f <= EPS32 * np.abs(ref_f))
    # the default float32 labels: half a float32 ulp of the label, in energy units, on top
    e32, _ = scaler.transform(y=(energy, force), X=numbers)
    back32, _ = scaler.inverse_transform(y=(e32, f_t), X=numbers)
    bar32 = 1e-12 * E + 0.5 * EPS32 * np.abs(e32.cpu().numpy().astype(np.float64)) * CASES["scale_" + tag]
    assert np.all(np.abs(back32.cpu().numpy() - ref_e) <= bar32)


def test_two_fits_and_a_fit_on_a_side_stream_give_identical_bits():
    first, numbers, energy, force = _fit("e")
    second, _, _, _ = _fit("e")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        from gcnn_keras_amd.data.transform.scaler import EnergyForceExtensiveLabelScaler
        side = EnergyForceExtensiveLabelScaler().fit(y=(energy, force), X=numbers)
        side_t = side.transform(y=(energy, force), X=numbers)
    stream.synchronize()
    w = first.get_weights()
    assert w == second.get_weights() == side.get_weights()
    main_t = first.transform(y=(energy, force), X=numbers)
    assert torch.equal(main_t[0], side_t[0]) and torch.equal(main_t[1].values, side_t[1].values)
    weighted = [_fit("d")[0].get_weights() for _ in range(2)]           # sample weights and the intercept path
    assert weighted[0] == weighted[1]


# ------------------------------------------------------------------------------------------------------------ input forms
@pytest.mark.parametrize("tag,dtype", [("b", "int64"), ("b", "float32"), ("d", "int32"), ("e", "int64")])
def test_tensor_form_and_numpy_list_form_give_identical_bits(tag, dtype):
    from gcnn_keras_amd.data.transform.scaler import EnergyForceExtensiveLabelScaler
    tensor_scaler, numbers, energy, force = _fit(tag, NUMBER_DTYPES[dtype])
    s = CASES["splits_" + tag]
    z_rows = _rows(CASES["numbers_" + tag].astype(NUMBER_DTYPES[dtype]), s)
    f_rows = _rows(CASES["force_" + tag], s)
    e_host = CASES["energy_" + tag]
    weight = CASES["weight_" + tag] if "weight_" + tag in CASES else None
    list_scaler = EnergyForceExtensiveLabelScaler(**CONFIG[tag])
    e_l, f_l = list_scaler.fit_transform(y=(e_host, f_rows), X=z_rows, sample_weight=weight)
    assert list_scaler.get_weights() == tensor_scaler.get_weights()
    e_t, f_t = tensor_scaler.transform(y=(energy, force), X=numbers)
    assert isinstance(e_l, np.ndarray) and e_l.dtype == np.float32 and len(f_l) == len(z_rows)
    assert np.array_equal(e_l, e_t.cpu().numpy())
    assert all(np.array_equal(a, b) for a, b in zip(f_l, f_t.numpy_rows()))
    back_l = list_scaler.inverse_transform(y=(e_l, f_l), X=z_rows)
    back_t = tensor_scaler.inverse_transform(y=(e_t, f_t), X=numbers)
    assert back_l[0].dtype == np.float64 and np.array_equal(back_l[0], back_t[0].cpu().numpy())
    assert all(np.array_equal(a, b) for a, b in zip(back_l[1], back_t[1].numpy_rows()))
    # the deprecated separate arguments (force.py:226-247) and the data set methods land on the same kernels
    e_d, f_d = list_scaler.transform(y=e_host, force=f_rows, atomic_number=z_rows)
    assert np.array_equal(e_d, e_l) and all(np.array_equal(a, b) for a, b in zip(f_d, f_l))
    dataset = [{"atomic_number": z, "energy": e, "force": f} for z, e, f in zip(z_rows, e_host, f_rows)]
    out = list_scaler.transform_dataset(dataset, copy_dataset=True)
    assert all(np.array_equal(g["energy"], e) and np.array_equal(g["force"], f) for g, e, f in zip(out, e_l, f_l))


def test_energy_only_label_scaler_matches_the_energy_force_scaler():
    from gcnn_keras_amd.data.transform.scaler import ExtensiveMolecularLabelScaler
    both, numbers, energy, force = _fit("d")
    label = ExtensiveMolecularLabelScaler(fit_intercept=True)
    y_t = label.fit_transform(y=energy, X=numbers, sample_weight=CASES["weight_d"])
    assert {k: v for k, v in label.get_weights().items()} == both.get_weights()
    assert torch.equal(y_t, both.transform(y=(energy, force), X=numbers)[0])
    back = label.inverse_transform(y=y_t, X=numbers)
    assert back.dtype == torch.float64 and torch.equal(back, both.inverse_transform(y=(y_t, force), X=numbers)[0])


def test_singular_matrix_without_regularisation_raises_value_error():
    from gcnn_keras_amd.data.transform.scaler import EnergyForceExtensiveLabelScaler
    # one molecule C4H4 and alpha = 0: A = [[16, 16], [16, 16]], whose second pivot is exactly 0 in floating point
    numbers = _ragged(np.array([1, 1, 1, 1, 6, 6, 6, 6], dtype=np.int64), np.array([0, 8]))
    energy = torch.full((1, 1), -4174.0, dtype=torch.float64, device="cuda")
    force = _ragged(np.zeros((8, 3), np.float32), np.array([0, 8]))
    with pytest.raises(ValueError, match="positive definite"):
        EnergyForceExtensiveLabelScaler(alpha=0.0).fit(y=(energy, force), X=numbers)
    scaler = EnergyForceExtensiveLabelScaler(alpha=1e-9).fit(y=(energy, force), X=numbers)     # ... and alpha mends it
    assert np.all(np.isfinite(scaler.ridge.coef_))


# --------------------------------------------------------------------------------------------------------------- training
def test_training_on_transformed_labels_and_inverse_transform_of_predictions():
    from gcnn_keras_amd.literature import Schnet
    from gcnn_keras_amd.model.force import EnergyForceModel
    b = synth.qm9_like_batch(40, seed=3)
    assert np.array_equal(b["node_number"].astype(np.int64), CASES["numbers_b"])
    scaler, numbers, energy, force = _fit("b")
    e_t, f_t = scaler.transform(y=(energy, force), X=numbers)
    model = Schnet.make_model(depth=3)
    model.set_weights(list(synth.schnet_params(seed=7, random_bias=True).values()))
    efm = EnergyForceModel(model_energy=model, coordinate_input=1, energy_output=0, output_as_dict=False,
                           output_to_tensor=False, output_squeeze_states=True)
    efm.compile(optimizer=torch.optim.SGD(efm.trainable_weights, lr=1e-4),
                loss=["mean_squared_error", "mean_squared_error"], clipnorm=1.0)
    x = [_ragged(b["node_number"], b["node_splits"]), _ragged(b["node_coordinates"], b["node_splits"]),
         _ragged(b["edge_indices"], b["edge_splits"])]
    hist = efm.fit(x, [e_t, f_t], batch_size=16, epochs=2, shuffle=False)
    losses = hist.history
    print("losses on scaled labels:", losses)
    assert all(np.all(np.isfinite(losses[k])) for k in ("loss", "energy_loss", "force_loss"))
    assert 1e-2 < losses["energy_loss"][0] < 1e2                     # of order 1; the raw labels give 1e9
    eng, frc = efm.predict(x, batch_size=16)
    e_back, f_back = scaler.inverse_transform(y=(eng, frc), X=numbers)
    coef, intercept, scale = _weights(scaler)
    sel = np.asarray(scaler.get_weights()["_fit_atom_selection"])
    offset = CASES["counts_b"][:, sel].astype(np.float64) @ coef.T + intercept
    want_e = eng.cpu().numpy().astype(np.float64) * scale + offset
    want_f = frc.values.cpu().numpy().astype(np.float64) * scale
    E = float(np.max(np.abs(want_e)))
    assert e_back.dtype == torch.float64 and np.max(np.abs(e_back.cpu().numpy() - want_e)) <= 1e-12 * E
    assert np.all(np.abs(f_back.values.cpu().numpy() - want_f) <= EPS32 * np.abs(want_f))


# --------------------------------------------------------------------------------------------------------------------- MD
def _golden_scaler(tag):
    from gcnn_keras_amd.data.transform.scaler import EnergyForceExtensiveLabelScaler
    scaler = EnergyForceExtensiveLabelScaler(**CONFIG[tag])
    scaler.set_weights({"scale_": CASES["scale_" + tag].tolist(), "_fit_atom_selection": CASES["selection_" + tag].tolist(),
                        "_fit_atom_selection_mask": CASES["mask_" + tag].tolist(), "coef_": CASES["coef_" + tag].tolist(),
                        "intercept_": 0.0, "n_features_in_": int(len(CASES["selection_" + tag]))})
    return scaler


def test_md_steps_with_the_scaler_postprocessor_on_the_device_and_on_the_host():
    from gcnn_keras_amd.graph.postprocessor import ExtensiveEnergyForceScalerPostprocessor
    from gcnn_keras_amd.moldyn import MolDynamicsModelPredictor
    from oracle import kgcnn_oracle as ko
    from oracle import torch_force_oracle as tfo
    from parity import assert_forces_close, assert_rows_close
    from test_gpu_moldyn import ITEMS, P, _graphs, _painn_ef
    model = _painn_ef()
    b = synth.md17_like_batch(num_graphs=1, seed=6)
    assert np.array_equal(b["node_number"].astype(np.int64), CASES["numbers_c"][:21])    # case c's composition
    post = ExtensiveEnergyForceScalerPostprocessor(_golden_scaler("c"))
    scale, offset = CASES["scale_c"], CASES["offset_c"][0]                                # the golden inverse transform
    outs = {"energy": "energy", "forces": "force"}
    plain = MolDynamicsModelPredictor(model=model, model_inputs=ITEMS, model_outputs=outs, use_graph=True)
    device = MolDynamicsModelPredictor(model=model, model_inputs=ITEMS, model_outputs=outs, use_graph=True,
                                       tensor_postprocessors=[post])
    host = MolDynamicsModelPredictor(model=model, model_inputs=ITEMS, model_outputs=outs, use_graph=True,
                                     graph_postprocessors=[post])
    rng = np.random.default_rng(0)
    xyz = b["node_coordinates"].copy()
    for step in range(3):
        raw, got_d, got_h = plain(_graphs(b, xyz)), device(_graphs(b, xyz)), host(_graphs(b, xyz))
        e_d, e_h = np.asarray(got_d[0]["energy"]), np.asarray(got_h[0]["energy"])
        f_d, f_h = np.asarray(got_d[0]["forces"]), np.asarray(got_h[0]["forces"])
        assert e_d.shape == e_h.shape == np.asarray(raw[0]["energy"]).shape and f_d.shape == f_h.shape == (21, 3)
        assert np.all(np.abs(e_d - e_h) <= EPS32 * np.abs(e_h)), "step %d energies" % step
        assert np.all(np.abs(f_d - f_h) <= EPS32 * np.abs(f_h)), "step %d forces" % step
        # the host form is the golden inverse transform of what the model returned
        e_raw = np.asarray(raw[0]["energy"], np.float64)
        assert np.all(np.abs(e_h - (e_raw * scale + offset)) <= 1e-12 * np.abs(e_h) + EPS32 * np.abs(e_raw) * scale)
        # tests/test_gpu_moldyn.py::_check_against_oracle's recipe, the oracle pushed through the golden inverse transform
        bb = dict(b, node_coordinates=np.asarray(xyz, np.float32))
        e_ref = [ko.painn_forward(ko.to_dtype(P, dt), ko.R(bb["node_number"], bb["node_splits"]),
                                  ko.R(bb["node_coordinates"].astype(dt), bb["node_splits"]),
                                  ko.R(bb["edge_indices"], bb["edge_splits"]), depth=3, equiv_method="eps")
                 for dt in (np.float32, np.float64)]
        f32, f64 = (tfo.painn_energy_force(P, bb, dt, equiv_method="eps")[1] for dt in (torch.float32, torch.float64))
        for name, out in (("device", got_d), ("host", got_h)):
            eng = np.asarray(out[0]["energy"], np.float64).reshape(1, -1)
            frc = np.asarray(out[0]["forces"], np.float64)
            what = "MD step %d, %s postprocessor" % (step, name)
            assert_rows_close((eng - offset) / scale, e_ref[0], e_ref[1], what=what + " energy, offset removed")
            assert_rows_close(eng, np.asarray(e_ref[0], np.float64) * scale + offset,
                              np.asarray(e_ref[1], np.float64) * scale + offset, what=what + " energy")
            assert_forces_close(frc, np.asarray(f32, np.float64) * scale, np.asarray(f64, np.float64) * scale,
                                bb["node_splits"], what=what + " forces")
        xyz = xyz + rng.normal(scale=0.01, size=xyz.shape).astype(np.float32)
    # the first step is the capture; the scaler changes neither count
    assert plain.fast_steps == device.fast_steps == host.fast_steps == 2
    assert plain.graph_captures == device.graph_captures == host.graph_captures == 1
    assert post.scaler.check_flags() == 0
