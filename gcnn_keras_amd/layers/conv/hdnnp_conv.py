"""Charge equilibration and electrostatics of HDNNP4th (mirror of kgcnn/layers/conv/hdnnp_conv.py:15-627) on the HIP
engine.

``CENTCharge`` solves one bordered linear system per molecule, ``[[A, 1], [1^T, 0]] [Q; lambda] = [chi; Qtot]`` over all
atom pairs of the molecule, on ``mp_cent_charge_f32`` (csrc/mp_cent.hip: the matrix built from coordinates and tables in
LDS, Cholesky + Schur complement in FP64, one wave per molecule) instead of the reference's padding, masks, scatters and
``tf.linalg.solve``.  ``ElectrostaticEnergyGaussCharge`` is ``mp_gauss_energy_f32``.  Their reverse rules are the
``CentCharge`` / ``GaussElectrostatics`` functions of ``gcnn_keras_amd.autograd`` (first order).  The QM/MM layers are
existing elementwise and pooling ops.

The tables are fixed and kept as plain attributes (not weights), as the ACSF layers keep theirs, so a model's
``trainable_weights`` holds its networks only: ``param_trainable=True``, ``use_physical_params=False``, ``add_eps=True``
and ``CENTCharge(output_to_tensor=True)`` raise ``NotImplementedError``.  At most ``MP_CENT_MAX_ATOMS`` (128) atoms per
molecule: a larger molecule raises ``ValueError`` before any launch.
"""
import numpy as np
import torch

from ... import _ffi
from ..base import GraphBaseLayer
from ..modules import binary_values
from ..pooling import PoolingNodes

# Covalent radii in pm for Z = 0..96 (Wikipedia, "Covalent radius"; Z = 0 is a placeholder 0), the source the reference
# cites (hdnnp_conv.py:84).
COVALENT_RADII_PM = np.array([
    0.0, 31, 28,
    128, 96, 84, 73, 71, 66, 57, 58,
    166, 141, 121, 111, 107, 105, 102, 106,
    203, 176, 170, 160, 153, 139, 139, 132, 126, 124, 132, 122, 122, 120, 119, 120, 120, 116,
    220, 195, 190, 175, 164, 154, 147, 146, 142, 139, 145, 144, 142, 139, 139, 138, 139, 140,
    244, 215, 207, 204, 203, 201, 199, 198, 198, 196, 194, 192, 192, 189, 190, 187, 175, 187, 170, 162, 151, 144,
    141, 136, 136, 132, 145, 146, 148, 140, 150, 150,
    260, 221, 215, 206, 200, 196, 190, 187, 180, 169])
# Chemical hardness in eV for Z = 0..96 (PNAS 10.1073/pnas.2117416119), the source the reference cites (:95).
HARDNESS_EV = np.array([
    0.0, 6.2, 8.8,
    2.2, 4.6, 3.8, 4.7, 7.1, 5.6, 6.1, 9.1,
    2.1, 4.0, 2.6, 3.3, 4.7, 3.8, 4.5, 7.7,
    2.3, 3.2, 3.2, 2.9, 3.2, 3.4, 4.0, 3.6, 3.3, 3.3, 3.8, 5.8, 3.0, 3.3, 4.5, 3.9, 4.2, 7.7,
    1.9, 3.1, 3.1, 2.9, 3.3, 3.5, 3.7, 3.7, 3.9, 4.1, 3.6, 5.4, 3.1, 3.1, 4.0, 3.6, 3.8, 6.8,
    1.8, 2.7, 2.4, 2.3, 2.5, 2.7, 2.5, 3.0, 3.0, 3.2, 3.2, 3.3, 3.3, 3.3, 3.1, 3.5, 3.2, 3.8, 3.1, 3.6, 3.7, 3.7,
    3.8, 3.5, 3.6, 5.8, 3.1, 3.4, 3.3, 3.6, 3.6, 6.1,
    1.8, 3.0, 2.8, 2.8, 3.1, 3.0, 3.1, 3.5, 3.3, 3.3])


def _device_table(layer, key, table, device):
    """float32 copy of a per-element table on ``device`` (uploaded once per layer)."""
    cache = layer.__dict__.setdefault("_device_tables", {})
    hit = cache.get(key)
    if hit is not None and hit[0] == device:
        return hit[1]
    t = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float32)).to(device)
    cache[key] = (device, t)
    return t


def _flat_values(x, width_name):
    """Values of a ragged ``(batch, [N])`` or ``(batch, [N], 1)`` tensor as ``(N,)``."""
    v = x.values
    if v.dim() == 2 and int(v.shape[1]) == 1:
        v = v.reshape(-1)
    if v.dim() != 1:
        raise ValueError("%s must have shape (batch, [N]) or (batch, [N], 1), got values %s" % (width_name,
                                                                                          tuple(v.shape)))
    if v.dtype != torch.float32:
        raise TypeError("%s must be float32, got %s" % (width_name, v.dtype))
    return v


def _atomic_numbers(n):
    z = n.values.reshape(-1)
    return z if z.dtype == torch.int64 else z.to(torch.int64)


class CentSpec:
    """One charge solve bound to a batch: atomic numbers, molecule splits, total charges and tables.  ``forward`` /
    ``grad`` are the two entry points of csrc/mp_cent.hip."""

    def __init__(self, layer, z, splits, qtot):
        self.z, self.splits, self.qtot = z.contiguous(), splits, qtot
        self.G, self.N = int(splits.shape[0]) - 1, int(z.shape[0])
        self.sigma = _device_table(layer, "sigma", layer.weight_sigma, z.device)
        self.hardness = _device_table(layer, "hardness", layer.weight_j, z.device)
        self.ntab = int(self.sigma.shape[0])

    def _head(self, xyz):
        return (_ffi.ptr(xyz), _ffi.ptr(self.z), _ffi.ptr(self.splits), self.G, self.N)

    def forward(self, chi, xyz):
        q = torch.empty((self.N, 1), dtype=torch.float32, device=xyz.device)
        _ffi.call("mp_cent_charge_f32", *self._head(xyz.contiguous()), _ffi.ptr(chi.contiguous()), _ffi.ptr(self.qtot),
                  _ffi.ptr(self.sigma), _ffi.ptr(self.hardness), self.ntab, _ffi.ptr(q), _ffi.stream())
        return q

    def grad(self, xyz, q, g, want_chi=True, want_x=True):
        chi_bar = torch.empty((self.N,), dtype=torch.float32, device=xyz.device) if want_chi else None
        x_bar = torch.empty((self.N, 3), dtype=torch.float32, device=xyz.device) if want_x else None
        if chi_bar is None and x_bar is None:
            return None, None
        _ffi.call("mp_cent_charge_grad_f32", *self._head(xyz.contiguous()), _ffi.ptr(q.contiguous()),
                  _ffi.ptr(g.contiguous()), _ffi.ptr(self.sigma), _ffi.ptr(self.hardness), self.ntab,
                  _ffi.ptr(chi_bar), _ffi.ptr(x_bar), _ffi.stream())
        return chi_bar, x_bar


def cent_charges(layer, n, chi, xyz, qtot):
    """Ragged charges ``(batch, [N], 1)`` of one CENT solve per molecule (on the tape when chi or xyz requires grad)."""
    from ...autograd import CentCharge, needs_grad
    _ffi.require_device(xyz.values, chi.values, xyz.row_splits)
    if xyz.values.dtype != torch.float32:
        raise TypeError("CENTCharge expects float32 coordinates, got %s" % xyz.values.dtype)
    splits = xyz.row_splits_host()
    counts = np.diff(splits)
    if counts.size and int(counts.max()) > _ffi.MP_CENT_MAX_ATOMS:
        raise ValueError("CENTCharge: a molecule of %d atoms exceeds the charge solve's bound of %d atoms per molecule "
                         "(MP_CENT_MAX_ATOMS)" % (int(counts.max()), _ffi.MP_CENT_MAX_ATOMS))
    chi_v = _flat_values(chi, "chi")
    if not torch.is_tensor(qtot):
        qtot = torch.as_tensor(np.asarray(qtot, dtype=np.float32), device=xyz.values.device)
    qt = qtot.reshape(-1)
    if qt.dtype != torch.float32:
        qt = qt.to(torch.float32)
    if int(qt.shape[0]) != xyz.nrows():
        raise ValueError("total charge has %d entries for %d molecules" % (int(qt.shape[0]), xyz.nrows()))
    spec = CentSpec(layer, _atomic_numbers(n), xyz.row_splits, qt.contiguous())
    x_v = xyz.values
    if needs_grad(chi_v, x_v):
        return xyz.with_values(CentCharge.apply(chi_v, x_v, spec))
    return xyz.with_values(spec.forward(chi_v, x_v))


class GaussSpec:
    """One electrostatic-energy call bound to a batch: atomic numbers, index plan, splits and the sigma table."""

    def __init__(self, layer, z, xyz, idx, sigma_table):
        self.plan = idx.index_plan(xyz)
        self.z, self.node_splits, self.edge_splits = z.contiguous(), xyz.row_splits, idx.row_splits
        self.G, self.N = xyz.nrows(), int(z.shape[0])
        self.sigma = sigma_table
        self.ntab = int(sigma_table.shape[0])
        self.mult = float(layer.multiplicity) if layer.multiplicity else 0.0

    def forward(self, q, xyz):
        e = torch.empty((self.G, 1), dtype=torch.float32, device=xyz.device)
        _ffi.call("mp_gauss_energy_f32", _ffi.ptr(xyz.contiguous()), _ffi.ptr(self.z), _ffi.ptr(q.contiguous()),
                  _ffi.ptr(self.node_splits), self.G, self.N, _ffi.ptr(self.plan.cols), self.plan.M,
                  _ffi.ptr(self.edge_splits), _ffi.ptr(self.sigma), self.ntab, self.mult, _ffi.ptr(e), _ffi.stream())
        return e

    def grad(self, q, xyz, g, want_q=True, want_x=True):
        q_bar = torch.empty((self.N,), dtype=torch.float32, device=xyz.device) if want_q else None
        x_bar = torch.empty((self.N, 3), dtype=torch.float32, device=xyz.device) if want_x else None
        if q_bar is None and x_bar is None:
            return None, None
        ptr0, perm0, _ = self.plan.csr(0)
        ptr1, perm1, _ = self.plan.csr(1)
        _ffi.call("mp_gauss_energy_grad_f32", _ffi.ptr(xyz.contiguous()), _ffi.ptr(self.z), _ffi.ptr(q.contiguous()),
                  _ffi.ptr(self.node_splits), self.G, self.N, _ffi.ptr(self.plan.cols), self.plan.M, _ffi.ptr(ptr0),
                  _ffi.ptr(perm0), _ffi.ptr(ptr1), _ffi.ptr(perm1), _ffi.ptr(self.sigma), self.ntab, self.mult,
                  _ffi.ptr(g.reshape(-1).contiguous()), _ffi.ptr(q_bar), _ffi.ptr(x_bar), _ffi.stream())
        return q_bar, x_bar


def gauss_energy(layer, n, q, xyz, idx):
    """Per-molecule electrostatic energy ``(batch, 1)`` (on the tape when q or xyz requires grad)."""
    from ...autograd import GaussElectrostatics, needs_grad
    _ffi.require_device(xyz.values, q.values, idx.values)
    if xyz.values.dtype != torch.float32:
        raise TypeError("ElectrostaticEnergyGaussCharge expects float32 coordinates, got %s" % xyz.values.dtype)
    if idx.values.dim() != 2 or int(idx.values.shape[-1]) != 2:
        raise ValueError("ElectrostaticEnergyGaussCharge expects index pairs (batch, [M], 2)")
    z = _atomic_numbers(n)
    spec = GaussSpec(layer, z, xyz, idx, _device_table(layer, "sigma", layer.weight_sigma, z.device))
    q_v, x_v = _flat_values(q, "q"), xyz.values
    if needs_grad(q_v, x_v):
        return GaussElectrostatics.apply(q_v, x_v, spec)
    return spec.forward(q_v, x_v)


def _check_params(use_physical_params, param_trainable):
    if param_trainable:
        raise NotImplementedError("trainable charge-equilibration parameters are not implemented (param_trainable=True)")
    if not use_physical_params:
        raise NotImplementedError("charge equilibration without the physical tables (use_physical_params=False) is not "
                                  "implemented")


class CENTCharge(GraphBaseLayer):
    r"""Charge equilibration of Ko et al. (2021) (kgcnn/layers/conv/hdnnp_conv.py:15-271): per molecule
    :math:`[[A, 1], [1^T, 0]] [Q; \lambda] = [\chi; Q_{tot}]`, :math:`A_{ii} = J_i + 1 / (\sigma_i \sqrt{\pi})`,
    :math:`A_{ij} = \mathrm{erf}(r_{ij} / (\sqrt{2} \gamma_{ij})) / r_{ij}`, :math:`\gamma_{ij} = \sqrt{\sigma_i^2 +
    \sigma_j^2}`.  Inputs ``[n (batch, [N]), chi (batch, [N], 1), xyz (batch, [N], 3), qtot (batch, 1)]``; output the
    ragged charges ``(batch, [N], 1)``.  Tables: sigma = 0.0188973 x covalent radius [pm] (Bohr), J = 0.037 / 0.529177 x
    hardness [eV]."""

    _default_radii = 0.0188973 * COVALENT_RADII_PM
    _default_hardness = 0.037 / 0.529177 * HARDNESS_EV
    _max_atomic_number = 97
    weight_gradients = True   # layers/base.py: the layer has no weights that train

    def __init__(self, output_to_tensor: bool = False, use_physical_params: bool = True, param_constraint=None,
                 param_regularizer=None, param_initializer="glorot_uniform", param_trainable: bool = False, **kwargs):
        GraphBaseLayer.__init__(self, **kwargs)
        _check_params(use_physical_params, param_trainable)
        if output_to_tensor:
            raise NotImplementedError("CENTCharge(output_to_tensor=True) (padded charges with the Lagrange multiplier) "
                                      "is not implemented")
        self.output_to_tensor = output_to_tensor
        self.use_physical_params = use_physical_params
        self.param_constraint, self.param_regularizer = param_constraint, param_regularizer
        self.param_initializer, self.param_trainable = param_initializer, param_trainable
        self.weight_j = np.asarray(self._default_hardness, dtype=np.float32)
        self.weight_sigma = np.asarray(self._default_radii, dtype=np.float32)

    def call(self, inputs, mask=None, **kwargs):
        n, chi, x = self.assert_ragged_input_rank(inputs[:3], mask=mask, ragged_rank=1)
        return cent_charges(self, n, chi, x, inputs[3])

    def get_config(self):
        config = GraphBaseLayer.get_config(self)
        config.update({"output_to_tensor": self.output_to_tensor, "use_physical_params": self.use_physical_params,
                       "param_constraint": self.param_constraint, "param_regularizer": self.param_regularizer,
                       "param_initializer": self.param_initializer, "param_trainable": self.param_trainable})
        return config


class ElectrostaticEnergyGaussCharge(GraphBaseLayer):
    r"""Electrostatic energy of Gaussian charges (kgcnn/layers/conv/hdnnp_conv.py:274-444): per molecule
    :math:`\frac{1}{mult} \sum_{(i,j)} q_i q_j \mathrm{erf}(r_{ij} / (\sqrt{2} \gamma_{ij})) / r_{ij} + \sum_i q_i^2 /
    (2 \sqrt{\pi} \sigma_i)` over the given index pairs; a falsy ``multiplicity`` means no division.  Inputs ``[n, q,
    xyz, ij]``, output ``(batch, 1)``.  Standalone, sigma = 0.01 x covalent radius [pm] (Angstrom)."""

    _default_radii = 0.01 * COVALENT_RADII_PM
    _max_atomic_number = 97
    weight_gradients = True

    def __init__(self, add_eps: bool = False, multiplicity: float = 2.0, use_physical_params: bool = True,
                 param_constraint=None, param_regularizer=None, param_initializer="glorot_uniform",
                 param_trainable: bool = False, _suppress_weight_initialization: bool = False, **kwargs):
        GraphBaseLayer.__init__(self, **kwargs)
        self._init_energy(add_eps, multiplicity, _suppress_weight_initialization)
        if not _suppress_weight_initialization:
            _check_params(use_physical_params, param_trainable)
            self.use_physical_params = use_physical_params
            self.param_constraint, self.param_regularizer = param_constraint, param_regularizer
            self.param_initializer, self.param_trainable = param_initializer, param_trainable
            self.weight_sigma = np.asarray(self._default_radii, dtype=np.float32)

    def _init_energy(self, add_eps, multiplicity, suppress):
        if add_eps:
            raise NotImplementedError("ElectrostaticEnergyGaussCharge with add_eps=True is not implemented")
        self.add_eps = add_eps
        self.multiplicity = multiplicity
        self._suppress_weight_initialization = suppress

    def call(self, inputs, mask=None, **kwargs):
        n, q, xyz, ij = self.assert_ragged_input_rank(inputs, mask=mask, ragged_rank=1)
        return gauss_energy(self, n, q, xyz, ij)

    def get_config(self):
        config = GraphBaseLayer.get_config(self)
        config.update({"add_eps": self.add_eps, "multiplicity": self.multiplicity,
                       "use_physical_params": self.use_physical_params, "param_constraint": self.param_constraint,
                       "param_regularizer": self.param_regularizer, "param_initializer": self.param_initializer,
                       "param_trainable": self.param_trainable,
                       "_suppress_weight_initialization": self._suppress_weight_initialization})
        return config


class ElectrostaticQMMMEnergyPointCharge(GraphBaseLayer):
    r"""QM/MM point-charge energy :math:`\sum_i Q_i \Phi_i` per molecule (kgcnn/layers/conv/hdnnp_conv.py:446-513):
    inputs ``[q (batch, [N], 1), esp (batch, [N])]``, output ``(batch, 1)``; the engine's broadcasting multiply and
    graph pooling."""

    weight_gradients = True

    def __init__(self, add_eps: bool = False, **kwargs):
        super().__init__(**kwargs)
        self.add_eps = add_eps   # unused, as in the reference
        self.layer_pool_nodes = PoolingNodes(pooling_method="sum")

    def call(self, inputs, mask=None, **kwargs):
        q, esp = self.assert_ragged_input_rank(inputs, mask=mask, ragged_rank=1)
        qv = q.values if q.values.dim() > 1 else q.values.unsqueeze(-1)
        ev = esp.values if esp.values.dim() > 1 else esp.values.unsqueeze(-1)
        return self.layer_pool_nodes(q.with_values(binary_values(_ffi.MP_MUL, qv, ev)))

    def get_config(self):
        config = super().get_config()
        config.update({"add_eps": self.add_eps})
        return config


class ElectrostaticQMMMForcePointCharge(GraphBaseLayer):
    r"""QM/MM point-charge force :math:`Q_i \partial \Phi_i / \partial r_i` (kgcnn/layers/conv/hdnnp_conv.py:516-577):
    inputs ``[q (batch, [N], 1), esp_grad (batch, [N], 3)]``, output ragged ``(batch, [N], 3)``."""

    weight_gradients = True

    def call(self, inputs, **kwargs):
        q, esp_grad = self.assert_ragged_input_rank(inputs, mask=None, ragged_rank=1)
        qv = q.values if q.values.dim() > 1 else q.values.unsqueeze(-1)
        return esp_grad.with_values(binary_values(_ffi.MP_MUL, qv, esp_grad.values))


class CENTChargePlusElectrostaticEnergy(CENTCharge, ElectrostaticEnergyGaussCharge):
    """``CENTCharge`` then ``ElectrostaticEnergyGaussCharge`` (kgcnn/layers/conv/hdnnp_conv.py:579-627).  As in the
    reference the energy's own table is suppressed, so the energy uses CENT's sigma table (Bohr), not the Angstrom one.
    Inputs ``[n, chi, xyz, ij, qtot]``; returns ``(charges (batch, [N], 1), energy (batch, 1))``."""

    weight_gradients = True

    def __init__(self, output_to_tensor: bool = False, use_physical_params: bool = True, param_constraint=None,
                 param_regularizer=None, param_initializer="glorot_uniform", param_trainable: bool = False,
                 add_eps: bool = False, multiplicity: float = 2.0, **kwargs):
        CENTCharge.__init__(self, output_to_tensor=output_to_tensor, use_physical_params=use_physical_params,
                            param_constraint=param_constraint, param_regularizer=param_regularizer,
                            param_initializer=param_initializer, param_trainable=param_trainable, **kwargs)
        self._init_energy(add_eps, multiplicity, True)

    def call(self, inputs, mask=None, **kwargs):
        n, chi, xyz, ij, qtot = inputs
        n, chi, xyz, ij = self.assert_ragged_input_rank([n, chi, xyz, ij], mask=mask, ragged_rank=1)
        q = cent_charges(self, n, chi, xyz, qtot)
        return q, gauss_energy(self, n, q, xyz, ij)

    def get_config(self):
        config = CENTCharge.get_config(self)
        config.update({"add_eps": self.add_eps, "multiplicity": self.multiplicity})
        return config
