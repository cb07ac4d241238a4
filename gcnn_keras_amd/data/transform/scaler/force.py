"""``EnergyForceExtensiveLabelScaler`` - mirror of kgcnn/data/transform/scaler/force.py:11-367 on the HIP engine.

Scales energies and forces jointly: ``X`` holds the atomic numbers, ``y = (energy, forces)``.  The offset removal and the
residual deviation are those of ``mol._ExtensiveMolecularScalerBase`` (FP64 on the device); ``transform`` /
``inverse_transform`` are ONE launch for energies and forces together (force.py:164-178, :207-222).

Two input forms, one implementation:

* device form - ``RaggedTensor`` numbers, an ``(n_samples, n_states)`` energy tensor, ``RaggedTensor`` forces
  ``(batch, [N], 3)`` or ``(batch, [N], 3, n_states)``: device tensors come back, nothing is read back;
* list form - the reference's lists of NumPy arrays: packed with the engine's packer, run through the same kernels, read
  back (energies as one array, forces as a list of arrays) with the reference's unknown-species warning.

Forward energies and all forces are float32, inverse energies float64 (``dtype`` overrides the energy type).  Units for
energy and forces must match.  ``standardize_coordinates=True`` raises ``NotImplementedError`` as in the reference.
``_plot_predict`` is left out: matplotlib is not a dependency of this package.
"""
import numpy as np
import torch

from ....ragged import RaggedTensor
from ...utils import ragged_tensor_from_nested_numpy
from .mol import _ExtensiveMolecularScalerBase, _is_device_form, _length


class EnergyForceExtensiveLabelScaler(_ExtensiveMolecularScalerBase):

    def __init__(self, standardize_coordinates: bool = False,
                 energy: str = "energy", force: str = "force", atomic_number: str = "atomic_number",
                 sample_weight: str = None, **kwargs):
        super(EnergyForceExtensiveLabelScaler, self).__init__(**kwargs)
        self._standardize_coordinates = standardize_coordinates
        if self._standardize_coordinates:
            raise NotImplementedError("Scaling of coordinates is not supported. This class is a pure label scaler.")
        self._use_separate_input_arguments = False
        self._energy = energy
        self._force = force
        self._atomic_number = atomic_number
        self._sample_weight = sample_weight

    # noinspection PyPep8Naming
    def fit(self, y=None, *, X=None, sample_weight=None, force=None, atomic_number=None):
        """``y = (energy, forces)``, ``X`` = atomic numbers; the deprecated separate ``force`` / ``atomic_number``
        arguments follow the reference's ``_verify_input``.  Only the energies and the numbers enter the fit."""
        X, y, force, atomic_number = self._verify_input(X, y, force, atomic_number)
        return self._fit(molecular_property=y, sample_weight=sample_weight, atomic_number=atomic_number)

    # noinspection PyPep8Naming
    def fit_transform(self, y=None, *, X=None, sample_weight=None, force=None, atomic_number=None, copy: bool = True):
        X, y, force, atomic_number = self._verify_input(X, y, force, atomic_number)
        self.fit(X=X, y=y, atomic_number=atomic_number, force=force, sample_weight=sample_weight)
        return self.transform(X=X, y=y, copy=copy, force=force, atomic_number=atomic_number)

    # noinspection PyPep8Naming
    def transform(self, y=None, *, X=None, force=None, atomic_number=None, copy: bool = True, dtype=None):
        """``((energy - offset) / scale, forces / scale)`` (force.py:164-178)."""
        X, y, force, atomic_number = self._verify_input(X, y, force, atomic_number)
        return self._energy_force(y, force, atomic_number, copy, False, dtype)

    # noinspection PyPep8Naming
    def inverse_transform(self, y=None, *, X=None, force=None, atomic_number=None, copy: bool = True, dtype=None):
        """``(energy * scale + offset, forces * scale)`` (force.py:207-222)."""
        X, y, force, atomic_number = self._verify_input(X, y, force, atomic_number)
        return self._energy_force(y, force, atomic_number, copy, True, dtype)

    def _energy_force(self, energy, force, atomic_number, copy, inverse, dtype):
        self._require_fit()
        if not (_length(energy) == _length(force) == _length(atomic_number)):
            raise ValueError("Energy, forces and atomic numbers do not match in length: %d, %d, %d."
                             % (_length(energy), _length(force), _length(atomic_number)))
        device_form = _is_device_form(atomic_number) and torch.is_tensor(energy) and isinstance(force, RaggedTensor)
        numbers = self._numbers(atomic_number)
        dev = numbers.values.device
        e_in = self._labels(energy, dev)
        if isinstance(force, RaggedTensor):
            f_in = force
        else:
            rows = [np.asarray(f) for f in force]
            f_in = ragged_tensor_from_nested_numpy(rows, dtype=np.float32, device=dev)
        e_out, f_out, _ = self._apply(numbers, e_in, f_in.values, inverse, energy_dtype=dtype)
        if device_form:
            return e_out, f_in.with_values(f_out)
        self._warn_unknown()
        e_host = e_out.cpu().numpy()
        f_host = f_in.with_values(f_out).numpy_rows()
        if not copy:            # the reference's in-place form (force.py:172-177, :216-221) where the rows can hold it
            for i in range(len(e_host)):
                if isinstance(energy, np.ndarray) or isinstance(energy[i], np.ndarray):
                    energy[i][...] = e_host[i]
                if isinstance(force[i], np.ndarray):
                    force[i][...] = f_host[i]
            return energy, force
        return e_host, f_host

    # noinspection PyPep8Naming
    def _verify_input(self, X, y, force, atomic_number):
        """force.py:226-247, with lengths that also read ragged and dense device tensors."""
        if y is None:
            raise ValueError("`EnergyForceExtensiveLabelScaler` requires 'y' argument, but got 'None'.")
        if force is not None:
            self._use_separate_input_arguments = True
            if _length(force) == _length(y):
                energy, forces = y, force
            elif _length(y) == 2:
                energy, forces = y[0], force
            else:
                raise ValueError("Energy and forces do not match.")
        else:
            self._use_separate_input_arguments = False
            energy, forces = y
        if atomic_number is not None:
            atoms = atomic_number
            x_input = X
        else:
            atoms = X
            x_input = None
        return x_input, energy, forces, atoms

    def get_config(self) -> dict:
        config = super(EnergyForceExtensiveLabelScaler, self).get_config()
        config.update({
            "standardize_coordinates": self._standardize_coordinates,
            "energy": self._energy,
            "force": self._force,
            "atomic_number": self._atomic_number,
            "sample_weight": self._sample_weight
        })
        return config

    def set_config(self, config: dict):
        if config["standardize_coordinates"]:
            raise NotImplementedError("Scaling of coordinates is not supported. This class is a pure label scaler.")
        self._standardize_coordinates = config["standardize_coordinates"]
        self._energy = config["energy"]
        self._force = config["force"]
        self._atomic_number = config["atomic_number"]
        self._sample_weight = config["sample_weight"]
        config_super = {key: value for key, value in config.items() if key not in [
            "standardize_coordinates", "energy", "force", "atomic_number", "sample_weight"]}
        return super(EnergyForceExtensiveLabelScaler, self).set_config(config_super)

    # ---- datasets of graph dicts (force.py:278-367) -----------------------------------------------------------------------
    def fit_dataset(self, dataset, **fit_params):
        atoms = self._atomic_number
        energy, force = self._energy, self._force
        return self.fit(
            X=[item[atoms] for item in dataset],
            y=([item[energy] for item in dataset], [item[force] for item in dataset]),
            sample_weight=[item[self._sample_weight] for item in dataset] if self._sample_weight is not None else None,
            **fit_params)

    def _dataset(self, dataset, copy, copy_dataset, inverse):
        atoms = self._atomic_number
        energy, force = self._energy, self._force
        if copy_dataset:
            dataset = dataset.copy()
        call = self.inverse_transform if inverse else self.transform
        out_energy, out_force = call(
            atomic_number=[graph[atoms] for graph in dataset],
            y=([graph[energy] for graph in dataset], [graph[force] for graph in dataset]), copy=copy)
        for graph, graph_energy, graph_force in zip(dataset, out_energy, out_force):
            graph[energy] = graph_energy
            graph[force] = graph_force
        return dataset

    def transform_dataset(self, dataset, copy: bool = True, copy_dataset: bool = False):
        return self._dataset(dataset, copy, copy_dataset, inverse=False)

    def inverse_transform_dataset(self, dataset, copy: bool = True, copy_dataset: bool = False):
        return self._dataset(dataset, copy, copy_dataset, inverse=True)

    def fit_transform_dataset(self, dataset, copy: bool = True, copy_dataset: bool = False, **fit_params):
        self.fit_dataset(dataset=dataset, **fit_params)
        return self.transform_dataset(dataset=dataset, copy=copy, copy_dataset=copy_dataset)
