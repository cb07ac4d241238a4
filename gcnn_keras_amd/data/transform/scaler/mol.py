"""``ExtensiveMolecularLabelScaler`` - mirror of kgcnn/data/transform/scaler/mol.py:10-352, 468-596 on the HIP engine.

A ridge regression of the molecular property on the per-molecule element counts removes the atomic offsets, the
residual's standard deviation rescales what is left (mol.py:38-74).  The scaler sits where the data is:

* device tensors in give device tensors out - ``RaggedTensor`` atomic numbers (int64, int32 or float32 values), an
  ``(n_samples, n_states)`` float64 / float32 label tensor, and whatever ``MemoryGraphList.tensor(...)`` returned;
* ``fit`` is one stream of launches (``csrc/mp_scaler.hip``: species counts, normal equations in fixed-order FP64
  chunks, a Cholesky solve in LDS, the two-pass residual deviation) behind which the weights are read back ONCE, because
  ``get_weights`` needs them on the host.  ``transform`` / ``inverse_transform`` are one launch and read nothing back;
  ``check_flags()`` reads the flag word on request;
* the reference's lists of NumPy arrays are packed with the engine's packer and go through the same kernels; the results
  are read back and the reference's unknown-species warning is printed.

There is no CPU implementation of ``fit``.  ``solver`` is the Cholesky of the normal equations (sklearn's ``"auto"`` for
dense input); ``positive=True`` and the other solvers raise ``NotImplementedError``.  A non-positive pivot raises
``ValueError`` (sklearn's SVD fallback for a singular matrix is not rebuilt; with ``alpha > 0`` the matrix is positive
definite).  ``_plot_predict`` of the reference is left out: matplotlib is not a dependency of this package.

``config`` and ``weights`` have the reference's JSON layout, so a ``scaler.json`` written by either side loads on the other.
"""
import json
import os

import numpy as np
import torch

from .... import _ffi
from ....ragged import RaggedTensor
from ...utils import ragged_tensor_from_nested_numpy

_NUMBER_KINDS = {torch.float32: _ffi.MP_DT_F32, torch.int32: _ffi.MP_DT_I32, torch.int64: _ffi.MP_DT_I64}
_REAL_KINDS = {torch.float32: _ffi.MP_DT_F32, torch.float64: _ffi.MP_DT_F64}
_Z = _ffi.MP_SCALER_MAX_NUMBER
_N_INT = 2 * _Z + 4          # mask (95) | selection (96) | status | flags | pad: a multiple of 8 bytes


class _Ridge:
    """What the reference keeps in ``self.ridge``: the parameters of ``sklearn.linear_model.Ridge`` (``get_params`` /
    ``set_params``) and the fitted ``coef_`` (n_states, n_species), ``intercept_`` and ``n_features_in_``."""
    _defaults = {"alpha": 1e-9, "copy_X": True, "fit_intercept": False, "max_iter": None, "positive": False,
                 "random_state": None, "solver": "auto", "tol": 1e-4}

    def __init__(self, **params):
        self._params = dict(self._defaults)
        self.set_params(**params)

    def get_params(self):
        return dict(sorted(self._params.items()))

    def set_params(self, **params):
        for key in params:
            if key not in self._defaults:
                raise TypeError("Ridge got an unexpected parameter %r" % key)
        merged = dict(self._params, **params)
        if merged["positive"]:
            raise NotImplementedError("Ridge(positive=True) needs the L-BFGS solver, which the engine does not have")
        if merged["solver"] not in ("auto", "cholesky"):
            raise NotImplementedError("the engine solves the normal equations by Cholesky: solver must be 'auto' or "
                                      "'cholesky', got %r" % (merged["solver"],))
        self._params = merged
        return self


def _length(x):
    if isinstance(x, RaggedTensor):
        return x.nrows()
    return int(x.shape[0]) if torch.is_tensor(x) else len(x)


def _is_device_form(x):
    return isinstance(x, RaggedTensor) or torch.is_tensor(x)


class _ExtensiveMolecularScalerBase:
    """Scaler base class for extensive properties like energy: removes a linear behaviour with additive atom
    contributions (mol.py:10-352)."""

    _attributes_list_sklearn = ["n_features_in_", "coef_", "intercept_", "n_iter_", "feature_names_in_"]
    _attributes_list_mol = ["scale_", "_fit_atom_selection", "_fit_atom_selection_mask"]
    _weights_written = ["n_features_in_", "coef_", "intercept_"]
    max_atomic_number = _Z

    def __init__(self, alpha: float = 1e-9, fit_intercept: bool = False, standardize_scale: bool = True, **kwargs):
        self.ridge = _Ridge(alpha=alpha, fit_intercept=fit_intercept, **kwargs)
        self._standardize_scale = standardize_scale
        self._fit_atom_selection_mask = None
        self._fit_atom_selection = None
        self.scale_ = None
        self._molecular_property = None
        self._atomic_number = None
        self._sample_weight = None
        self._device = None        # device copies of the weights: table, present, intercept, scale, flags
        self._fit_flags = 0
        self.device = "cuda"

    # ---- inputs -----------------------------------------------------------------------------------------------------
    def _numbers(self, atomic_number):
        """Ragged atomic numbers on the device: a ``RaggedTensor`` as it is, a list of arrays through the packer."""
        if isinstance(atomic_number, RaggedTensor):
            _ffi.require_device(atomic_number.values, atomic_number.row_splits)
            if atomic_number.values.dtype not in _NUMBER_KINDS:
                atomic_number = atomic_number.with_values(atomic_number.values.to(torch.float32))
            if atomic_number.values.dim() != 1:
                atomic_number = atomic_number.with_values(atomic_number.values.reshape(-1))
            return atomic_number
        rows = [np.asarray(a).reshape(-1) for a in atomic_number]
        kind = next((r.dtype.kind for r in rows if len(r)), "i")
        return ragged_tensor_from_nested_numpy(rows, dtype=np.float32 if kind == "f" else np.int64, device=self.device)

    def _labels(self, y, device):
        """(n_samples, n_states) float64 / float32 labels on the device."""
        if not torch.is_tensor(y):
            y = np.asarray(y)
            if y.dtype != np.float32:
                y = y.astype(np.float64)
            y = torch.from_numpy(np.ascontiguousarray(y)).to(device)
        _ffi.require_device(y)
        if y.dtype not in _REAL_KINDS:
            y = y.to(torch.float64)
        if y.dim() != 2:
            raise ValueError("labels must have shape (n_samples, n_states), got %s" % (tuple(y.shape),))
        return y.contiguous()

    # ---- fit --------------------------------------------------------------------------------------------------------
    def _fit(self, molecular_property, atomic_number, sample_weight=None):
        """mol.py:38-74 on the device; the one read-back of the weights ends it."""
        if _length(atomic_number) != _length(molecular_property):
            raise ValueError("`ExtensiveMolecularScaler` different input shape '{0}' vs. '{1}'.".format(
                _length(atomic_number), _length(molecular_property)))
        numbers = self._numbers(atomic_number)
        dev = numbers.values.device
        y = self._labels(molecular_property, dev)
        G, S = int(y.shape[0]), int(y.shape[1])
        if G < 1 or not 1 <= S <= _ffi.MP_SCALER_MAX_STATES:
            raise ValueError("fit needs at least one sample and 1..%d states" % _ffi.MP_SCALER_MAX_STATES)
        w = None
        if sample_weight is not None:
            w = sample_weight if torch.is_tensor(sample_weight) else torch.from_numpy(
                np.asarray(sample_weight, dtype=np.float64).reshape(-1)).to(dev)
            w = w.to(torch.float64).reshape(-1).contiguous()
            if int(w.shape[0]) != G:
                raise ValueError("sample_weight must hold one weight per sample")
        params = self.ridge.get_params()
        fit_intercept = int(bool(params["fit_intercept"]))

        # one block: what is read back first (coef | intercept | scale | mask, selection, status, flags), then the rest
        n_head = _Z * S + 2 * S
        n_f64 = n_head + _N_INT // 2 + _Z * S + (_Z + S) + _Z * _Z + _Z * S
        raw = torch.zeros(n_f64, dtype=torch.float64, device=dev)
        coef, intercept, scale = raw[:_Z * S], raw[_Z * S:_Z * S + S], raw[_Z * S + S:n_head]
        ints = raw[n_head:n_head + _N_INT // 2].view(torch.int32)
        mask, sel, status, flags = ints[:_Z], ints[_Z:2 * _Z + 1], ints[2 * _Z + 1:2 * _Z + 2], ints[2 * _Z + 2:2 * _Z + 3]
        rest = raw[n_head + _N_INT // 2:]
        table, mean = rest[:_Z * S], rest[_Z * S:_Z * S + _Z + S]
        A = rest[_Z * S + _Z + S:_Z * S + _Z + S + _Z * _Z]
        b = rest[_Z * S + _Z + S + _Z * _Z:]
        counts = torch.empty((G, _Z), dtype=torch.int32, device=dev)
        ws_bytes = _ffi.workspace_bytes("mp_scaler_fit_ws_bytes", G, S)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        st = _ffi.stream()
        _ffi.call("mp_scaler_species_count", _ffi.ptr(numbers.values), _NUMBER_KINDS[numbers.values.dtype],
                  _ffi.ptr(numbers.row_splits), G, int(numbers.values.shape[0]), _ffi.ptr(counts), _ffi.ptr(mask),
                  _ffi.ptr(sel), _ffi.ptr(flags), st)
        _ffi.call("mp_scaler_normal_f64", _ffi.ptr(counts), _ffi.ptr(sel), G, _ffi.ptr(y), _REAL_KINDS[y.dtype], S,
                  _ffi.ptr(w), float(params["alpha"]), fit_intercept, _ffi.ptr(A), _ffi.ptr(b), _ffi.ptr(mean),
                  _ffi.ptr(ws), ws_bytes, st)
        _ffi.call("mp_scaler_solve_f64", _ffi.ptr(A), _ffi.ptr(b), _ffi.ptr(mean), _ffi.ptr(sel), S, fit_intercept,
                  _ffi.ptr(coef), _ffi.ptr(intercept), _ffi.ptr(table), _ffi.ptr(status), st)
        _ffi.call("mp_scaler_residual_std_f64", _ffi.ptr(counts), _ffi.ptr(sel), G, _ffi.ptr(y), _REAL_KINDS[y.dtype], S,
                  _ffi.ptr(coef), _ffi.ptr(intercept), int(bool(self._standardize_scale)), _ffi.ptr(scale),
                  _ffi.ptr(ws), ws_bytes, st)
        head = raw[:n_head + _N_INT // 2].cpu()                     # the one synchronisation of the scaler
        head_int = head[n_head:].view(torch.int32).numpy()
        head = head.numpy()
        if int(head_int[2 * _Z + 1]) != 0:
            raise ValueError("ridge normal matrix is not positive definite (pivot %d): raise alpha"
                             % (int(head_int[2 * _Z + 1]) - 1))
        K = int(head_int[2 * _Z])
        self._fit_flags = int(head_int[2 * _Z + 2])
        self._fit_atom_selection = head_int[_Z:_Z + K].astype(np.int64)
        self._fit_atom_selection_mask = head_int[:_Z].astype(bool)
        self.ridge.coef_ = np.ascontiguousarray(head[:_Z * S].reshape(_Z, S)[:K].T)
        self.ridge.intercept_ = head[_Z * S:_Z * S + S].copy() if fit_intercept else 0.0
        self.ridge.n_features_in_ = K
        self.scale_ = head[_Z * S + S:n_head].copy()
        self._device = {"device": dev, "S": S, "table": table, "present": mask, "intercept": intercept, "scale": scale,
                        "flags": torch.zeros(1, dtype=torch.int32, device=dev), "keep": raw}
        return self

    # ---- weights on the host and on the device --------------------------------------------------------------------------
    def _require_fit(self):
        if self._fit_atom_selection_mask is None or getattr(self.ridge, "coef_", None) is None:
            raise ValueError("`ExtensiveMolecularScaler` has not been fitted yet. Can not predict.")

    def _host_weights(self):
        """``(selection (K), coef (S, K), intercept (S), scale (S))`` as float64 arrays."""
        self._require_fit()
        coef = np.asarray(self.ridge.coef_, dtype=np.float64)
        coef = coef.reshape(1, -1) if coef.ndim < 2 else coef
        S = coef.shape[0]
        intercept = np.broadcast_to(np.asarray(self.ridge.intercept_, dtype=np.float64).reshape(-1), (S,)).copy()
        if self._standardize_scale:
            scale = np.broadcast_to(np.asarray(self.scale_, dtype=np.float64).reshape(-1), (S,)).copy()
        else:
            scale = np.ones(S)
        sel = np.asarray(self._fit_atom_selection, dtype=np.int64).reshape(-1)
        return sel, coef, intercept, scale

    def _device_state(self, dev):
        st = self._device
        if st is not None and st["device"] == dev:
            return st
        sel, coef, intercept, scale = self._host_weights()
        S = coef.shape[0]
        table = np.zeros((_Z, S))
        table[sel] = coef.T
        present = np.zeros(_Z, dtype=np.int32)
        present[sel] = 1
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
        self._device = {"device": dev, "S": S, "table": up(table).reshape(-1), "present": up(present),
                        "intercept": up(intercept), "scale": up(scale),
                        "flags": torch.zeros(1, dtype=torch.int32, device=dev)}
        return self._device

    def check_flags(self):
        """The ``MP_FLAG_*`` word of the fit and of every transform since (one read-back): ``MP_FLAG_OOB`` for an atomic
        number outside [0, 95), ``MP_FLAG_UNKNOWN_SPECIES`` for a species the fit did not see (it contributed 0)."""
        word = self._fit_flags
        if self._device is not None:
            word |= int(self._device["flags"].item())
        return word

    def _apply(self, numbers, energy, force, inverse, energy_dtype=None, want_offset=False):
        """One ``mp_scaler_apply`` launch: ``(energy_out, force_values_out, offset)`` on the device, nothing read back.
        ``energy``: (G, S) tensor or None; ``force``: flat (N, 3[, S]) float32 values or None."""
        self._require_fit()
        dev = numbers.values.device
        st = self._device_state(dev)
        S, G, N = st["S"], numbers.nrows(), int(numbers.values.shape[0])
        e_out = f_out = offset = None
        e_kind = o_kind = 0
        if energy is not None:
            if energy.dtype not in _REAL_KINDS:
                energy = energy.to(torch.float64)
            energy = energy.contiguous()
            if energy.numel() != G * S:
                raise ValueError("energies of shape %s do not hold %d samples x %d states" % (tuple(energy.shape), G, S))
            out_dtype = energy_dtype or (torch.float64 if inverse else torch.float32)
            e_out = torch.empty(energy.shape, dtype=out_dtype, device=dev)
            e_kind, o_kind = _REAL_KINDS[energy.dtype], _REAL_KINDS[out_dtype]
        if force is not None:
            force = force.to(torch.float32).contiguous()
            if force.numel() != N * 3 * S:
                raise ValueError("forces of shape %s do not hold %d atoms x 3 x %d states" % (tuple(force.shape), N, S))
            f_out = torch.empty_like(force)
        if want_offset:
            offset = torch.empty((G, S), dtype=torch.float64, device=dev)
        _ffi.call("mp_scaler_apply", _ffi.ptr(numbers.values), _NUMBER_KINDS[numbers.values.dtype],
                  _ffi.ptr(numbers.row_splits), G, N, S, int(bool(inverse)), _ffi.ptr(st["table"]),
                  _ffi.ptr(st["present"]), _ffi.ptr(st["intercept"]), _ffi.ptr(st["scale"]), _ffi.ptr(energy), e_kind,
                  _ffi.ptr(e_out), o_kind, _ffi.ptr(force), _ffi.ptr(f_out), _ffi.ptr(offset), _ffi.ptr(st["flags"]),
                  _ffi.stream())
        return e_out, f_out, offset

    def _warn_unknown(self):
        """List form only (the results are read back anyway): the reference's warning, mol.py:93-94."""
        flags = self._device["flags"]
        word = int(flags.item())
        if word:
            self._fit_flags |= word          # kept for check_flags(); the device word starts over
            flags.zero_()
        if word & _ffi.MP_FLAG_UNKNOWN_SPECIES:
            print("`ExtensiveMolecularScaler` got unknown atom species in transform.")

    def _predict(self, atomic_number):
        """Offsets ``(n_samples, n_states)`` in FP64 (mol.py:76-98): a device tensor for device numbers, an array for a
        list of arrays."""
        self._require_fit()
        device_form = _is_device_form(atomic_number)
        _, _, offset = self._apply(self._numbers(atomic_number), None, None, False, want_offset=True)
        if device_form:
            return offset
        self._warn_unknown()
        return offset.cpu().numpy()

    def _transform(self, molecular_property, atomic_number, copy=True, inverse=False, dtype=None):
        """mol.py:121-140 / :157-177.  Forward gives float32 labels of order 1, the inverse float64 (``dtype`` overrides)."""
        self._require_fit()
        if _length(atomic_number) != _length(molecular_property):
            raise ValueError("`ExtensiveMolecularScaler` different input shape '{0}' vs. '{1}'.".format(
                _length(atomic_number), _length(molecular_property)))
        device_form = _is_device_form(atomic_number)
        numbers = self._numbers(atomic_number)
        y = self._labels(molecular_property, numbers.values.device)
        out, _, _ = self._apply(numbers, y, None, inverse, energy_dtype=dtype)
        if device_form and torch.is_tensor(molecular_property):
            return out
        self._warn_unknown()
        out = out.cpu().numpy()
        if not copy and isinstance(molecular_property, np.ndarray):
            molecular_property[...] = out
            return molecular_property
        return out

    def _fit_transform(self, molecular_property, atomic_number, copy=True, sample_weight=None):
        self._fit(molecular_property=molecular_property, atomic_number=atomic_number, sample_weight=sample_weight)
        return self._transform(molecular_property=molecular_property, atomic_number=atomic_number, copy=copy)

    def _inverse_transform(self, molecular_property, atomic_number, copy=True, dtype=None):
        return self._transform(molecular_property, atomic_number, copy=copy, inverse=True, dtype=dtype)

    # ---- serialisation (mol.py:179-264) ---------------------------------------------------------------------------------
    def get_config(self) -> dict:
        config = {}
        config.update(self.ridge.get_params())
        config.update({"standardize_scale": self._standardize_scale})
        return config

    def set_config(self, config):
        self._standardize_scale = config["standardize_scale"]
        self.ridge.set_params(**{key: value for key, value in config.items() if key not in ["standardize_scale"]})
        self._device = None
        return self

    def get_weights(self) -> dict:
        weights = dict()
        for x in self._attributes_list_mol:
            weights.update({x: np.array(getattr(self, x)).tolist()})
        for x in self._weights_written:
            if hasattr(self.ridge, x):
                weights.update({x: np.array(getattr(self.ridge, x)).tolist()})
        return weights

    def set_weights(self, weights: dict):
        for item, value in weights.items():
            if item in self._attributes_list_mol:
                setattr(self, item, np.array(value))
            elif item in self._attributes_list_sklearn:
                setattr(self.ridge, item, np.array(value))
            else:
                print("`ExtensiveMolecularScaler` got unknown weight '%s'." % item)
        self._device = None
        self._fit_flags = 0

    def save_weights(self, file_path: str):
        weights = {key: np.array(value) for key, value in self.get_weights().items()}
        np.savez(os.path.splitext(file_path)[0] + ".npz", **weights)

    def get_scaling(self):
        """Scale of shape (1, n_properties)."""
        if self.scale_ is None:
            return
        return np.expand_dims(self.scale_, axis=0)

    def save(self, file_path: str):
        full_info = {"class_name": type(self).__name__, "module_name": type(self).__module__,
                     "config": self.get_config(), "weights": self.get_weights()}
        with open(os.path.splitext(file_path)[0] + ".json", "w") as json_file:
            json.dump(full_info, json_file)

    def load(self, file_path: str):
        with open(file_path, "r") as json_file:
            full_info = json.load(json_file)
        self.set_config(full_info["config"])
        self.set_weights(full_info["weights"])
        return self

    # ---- datasets of graph dicts (mol.py:268-351) -------------------------------------------------------------------------
    def fit_dataset(self, dataset):
        return self._fit(
            molecular_property=np.array([item[self._molecular_property] for item in dataset]),
            atomic_number=[item[self._atomic_number] for item in dataset],
            sample_weight=[item[self._sample_weight] for item in dataset] if self._sample_weight is not None else None)

    def _dataset(self, dataset, copy, copy_dataset, inverse):
        if copy_dataset:
            dataset = dataset.copy()
        out = self._transform(
            molecular_property=np.array([item[self._molecular_property] for item in dataset]),
            atomic_number=[item[self._atomic_number] for item in dataset], copy=copy, inverse=inverse)
        for graph, out_value in zip(dataset, out):
            graph[self._molecular_property] = out_value
        return dataset

    def transform_dataset(self, dataset, copy: bool = True, copy_dataset: bool = False):
        return self._dataset(dataset, copy, copy_dataset, inverse=False)

    def inverse_transform_dataset(self, dataset, copy: bool = True, copy_dataset: bool = False):
        return self._dataset(dataset, copy, copy_dataset, inverse=True)

    def fit_transform_dataset(self, dataset, copy: bool = True, copy_dataset: bool = False):
        self.fit_dataset(dataset=dataset)
        return self.transform_dataset(dataset=dataset, copy=copy, copy_dataset=copy_dataset)


class ExtensiveMolecularLabelScaler(_ExtensiveMolecularScalerBase):
    """Extensive scaler for labels (mol.py:468-596): ``y`` holds the labels ``(n_samples, n_labels)``, ``X`` (or
    ``atomic_number``) the atomic numbers.

    .. code-block:: python

        scaler = ExtensiveMolecularLabelScaler()
        scaler.fit(X=mol_num, y=data)               # lists of arrays, or RaggedTensor numbers + a device tensor
        scaled = scaler.transform(X=mol_num, y=data)
        scaler.save("example.json")
    """

    # noinspection PyPep8Naming
    def __init__(self, y: str = "graph_labels", atomic_number: str = "atomic_number", sample_weight: str = None,
                 **kwargs):
        super(ExtensiveMolecularLabelScaler, self).__init__(**kwargs)
        self._molecular_property = y
        self._atomic_number = atomic_number
        self._sample_weight = sample_weight

    def _assert_has_y(self, y):
        if y is None:
            raise ValueError("Require labels in `y` for `%s`. Input must be e.g. 'fit(y=data)'." % type(self).__name__)

    # noinspection PyPep8Naming
    def fit(self, y=None, *, X=None, sample_weight=None, atomic_number=None):
        self._assert_has_y(y)
        atomic_number = atomic_number if atomic_number is not None else X
        return self._fit(molecular_property=y, sample_weight=sample_weight, atomic_number=atomic_number)

    # noinspection PyPep8Naming
    def transform(self, y=None, *, X=None, copy=True, atomic_number=None):
        self._assert_has_y(y)
        atomic_number = atomic_number if atomic_number is not None else X
        return self._transform(molecular_property=y, atomic_number=atomic_number, copy=copy)

    # noinspection PyPep8Naming
    def fit_transform(self, y=None, *, X=None, copy=True, atomic_number=None, sample_weight=None):
        self.fit(y=y, X=X, sample_weight=sample_weight, atomic_number=atomic_number)
        return self.transform(y=y, X=X, copy=copy, atomic_number=atomic_number)

    # noinspection PyPep8Naming
    def inverse_transform(self, y=None, *, X=None, copy=True, atomic_number=None):
        self._assert_has_y(y)
        atomic_number = atomic_number if atomic_number is not None else X
        return self._inverse_transform(molecular_property=y, atomic_number=atomic_number, copy=copy)

    def get_config(self):
        config = super(ExtensiveMolecularLabelScaler, self).get_config()
        config.update({"y": self._molecular_property, "atomic_number": self._atomic_number,
                       "sample_weight": self._sample_weight})
        return config

    def set_config(self, config):
        keys = ["y", "atomic_number", "sample_weight"]
        super(ExtensiveMolecularLabelScaler, self).set_config({k: v for k, v in config.items() if k not in keys})
        self._molecular_property = config["y"]
        self._atomic_number = config["atomic_number"]
        self._sample_weight = config["sample_weight"]
        return self
