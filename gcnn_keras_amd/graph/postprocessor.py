"""Graph postprocessors - mirror of kgcnn/graph/postprocessor.py:6-37.

``ExtensiveEnergyForceScalerPostprocessor`` puts the inverse transform of a fitted ``EnergyForceExtensiveLabelScaler``
behind a model, in two forms:

* host form - a member of ``MolDynamicsModelPredictor(graph_postprocessors=[...])``: the reference's callable on
  ``(graph, pre_graph)``, plain NumPy float64 from the scaler's weights, one molecule at a time (``np.unique`` and the
  ridge prediction of kgcnn/data/transform/scaler/mol.py:76-98).  It needs no GPU;
* device form - a member of ``MolDynamicsModelPredictor(tensor_postprocessors=[...])``: ``call_tensors`` is one
  ``mp_scaler_apply`` launch on the model's output tensors, in front of the read-back the step does anyway.
"""
import numpy as np
import torch

from ..ragged import RaggedTensor


class ExtensiveEnergyForceScalerPostprocessor:
    """Inverse-transform energies and forces of an output graph; the atomic numbers come from the input graph.

    Args:
        scaler: fitted ``EnergyForceExtensiveLabelScaler``.
        energy (str): name of the energy property of the output graph. Default is 'energy'.
        force (str): name of the force property of the output graph. Default is 'forces'.
        atomic_number (str): name of the atomic numbers in the input graph. Default is 'node_number'.
        energy_dtype: type of the device form's energies, float64 by default (a total energy of 4e4 eV does not fit
            float32; the host form returns float64 as well).
    """

    def __init__(self, scaler, energy: str = "energy", force: str = "forces", atomic_number: str = "node_number",
                 name="extensive_energy_force_scaler", energy_dtype=torch.float64):
        if isinstance(scaler, dict):
            raise TypeError("serialized scalers are not resolved on this engine: pass the scaler object")
        self.scaler = scaler
        self.name = name
        self.energy_dtype = energy_dtype
        self._to_obtain_pre = {"atomic_number": atomic_number}
        self._to_obtain = {"y": energy, "force": force}
        self._to_assign = [energy, force]

    # ---- host form ------------------------------------------------------------------------------------------------------
    def call(self, y, force, atomic_number):
        """One molecule in NumPy float64 (postprocessor.py:32-37 through force.py:207-222)."""
        sel, coef, intercept, scale = self.scaler._host_weights()
        unique, num = np.unique(np.asarray(atomic_number).astype(np.int64), return_counts=True)
        array_atoms = np.zeros(self.scaler.max_atomic_number)
        array_atoms[unique] = num
        positives = array_atoms[sel]
        if np.sum(positives) != np.sum(num):
            print("`ExtensiveMolecularScaler` got unknown atom species in transform.")
        offset = positives @ coef.T + intercept
        energy = np.asarray(y, dtype=np.float64) * scale + offset
        forces = np.asarray(force, dtype=np.float64) * scale
        return energy, forces

    def __call__(self, graph, pre_graph):
        energy, forces = self.call(graph[self._to_obtain["y"]], graph[self._to_obtain["force"]],
                                   pre_graph[self._to_obtain_pre["atomic_number"]])
        return {self._to_assign[0]: energy, self._to_assign[1]: forces}

    # ---- device form ----------------------------------------------------------------------------------------------------
    def call_tensors(self, outputs, inputs):
        """``outputs``: the model's output tensors by name, ``inputs``: its input tensors by name.  Returns the replaced
        outputs; one launch, nothing read back."""
        energy, force = outputs[self._to_obtain["y"]], outputs[self._to_obtain["force"]]
        numbers = self.scaler._numbers(inputs[self._to_obtain_pre["atomic_number"]])
        ragged = isinstance(force, RaggedTensor)
        values = (force.values if ragged else force).detach()
        e_out, f_out, _ = self.scaler._apply(numbers, energy.detach(), values, True, energy_dtype=self.energy_dtype)
        return {self._to_assign[0]: e_out, self._to_assign[1]: force.with_values(f_out) if ragged else f_out}
