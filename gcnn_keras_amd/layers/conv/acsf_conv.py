"""Atom-centred symmetry functions of HDNNP2nd (mirror of kgcnn/layers/conv/acsf_conv.py:16-546) on the HIP engine.

``ACSFG2`` / ``ACSFG4`` run ``mp_acsf_g2_f32`` / ``mp_acsf_g4_f32`` (csrc/mp_acsf.hip): one receiver-parallel launch per
call instead of the reference's gathers, per-bond parameter lookups, products and relational scatter.  Their reverse to
the coordinates and, for training through forces, their forward-mode derivative are the ``ACSF`` rules of
``gcnn_keras_amd.autograd``.

The parameter tables are fixed: ``param_trainable=True`` raises ``NotImplementedError``.  They are kept as plain
attributes (not weights), so a model's ``trainable_weights`` holds the network's weights only.
"""
import numpy as np
import torch

from ... import _ffi
from ..base import GraphBaseLayer
from ..modules import binary_values

_MAX_Z = 31


def _device_tables(layer, device):
    """(params, rmap, pmap) of a layer on ``device`` (uploaded once)."""
    cache = layer.__dict__.get("_tables")
    if cache is not None and cache[0] == device:
        return cache[1]

    def as_map(a):
        m = np.asarray(a, dtype=np.int64)
        return torch.from_numpy(np.where((m >= 0) & (m < np.iinfo(np.int32).max), m, -1).astype(np.int32)).to(device)

    params = torch.from_numpy(np.ascontiguousarray(layer._param_table, dtype=np.float32)).to(device)
    rmap = as_map(layer.reverse_mapping)
    pmap = as_map(layer.reverse_pair_mapping).reshape(-1) if hasattr(layer, "reverse_pair_mapping") else None
    tables = (params, rmap, pmap)
    layer.__dict__["_tables"] = (device, tables)
    return tables


class AcsfSpec:
    """One ACSF call bound to a batch: atomic numbers, index plan, tables.  ``forward`` / ``grad`` / ``jvp`` are the three
    entry points of csrc/mp_acsf.hip on coordinates (N, 3)."""

    def __init__(self, layer, z, plan):
        self.g4 = isinstance(layer, ACSFG4)
        self.K = 3 if self.g4 else 2
        self.z = z
        self.plan = plan
        self.params, self.rmap, self.pmap = _device_tables(layer, z.device)
        self.nrel, self.nfun = layer.num_relations, layer.num_functions
        self.ncenter = layer.num_centers
        self.mult = float(layer.multiplicity) if (self.g4 and layer.multiplicity is not None) else 0.0
        self.width = self.nrel * self.nfun

    def _csr(self, c):
        ptr, perm, _ = self.plan.csr(c)
        return _ffi.ptr(ptr), _ffi.ptr(perm)

    def _head(self, xyz):
        return (_ffi.ptr(xyz), _ffi.ptr(self.z), self.plan.N, _ffi.ptr(self.plan.cols), self.plan.M)

    def _table(self):
        if self.g4:
            return (_ffi.ptr(self.rmap), _ffi.ptr(self.pmap), _ffi.ptr(self.params), self.nrel, self.nfun,
                    self.ncenter, self.mult)
        return (_ffi.ptr(self.rmap), _ffi.ptr(self.params), self.nrel, self.nfun, self.ncenter)

    def forward(self, xyz):
        xyz = xyz.contiguous()
        out = torch.empty((self.plan.N, self.width), dtype=torch.float32, device=xyz.device)
        name = "mp_acsf_g4_f32" if self.g4 else "mp_acsf_g2_f32"
        _ffi.call(name, *self._head(xyz), *self._csr(0), *self._table(), _ffi.ptr(out), _ffi.stream())
        return out

    def jvp(self, xyz, h):
        xyz, h = xyz.contiguous(), h.contiguous()
        out = torch.empty((self.plan.N, self.width), dtype=torch.float32, device=xyz.device)
        name = "mp_acsf_g4_jvp_f32" if self.g4 else "mp_acsf_g2_jvp_f32"
        _ffi.call(name, *self._head(xyz), *self._csr(0), *self._table(), _ffi.ptr(h), _ffi.ptr(out), _ffi.stream())
        return out

    def grad(self, xyz, g):
        xyz, g = xyz.contiguous(), g.contiguous()
        dx = torch.empty((self.plan.N, 3), dtype=torch.float32, device=xyz.device)
        ws, nbytes = _ffi.float_workspace("mp_acsf_grad_ws_bytes", self.plan.M, self.K, device=xyz.device)
        csr = []
        for c in range(self.K):
            csr.extend(self._csr(c))
        name = "mp_acsf_g4_grad_f32" if self.g4 else "mp_acsf_g2_grad_f32"
        _ffi.call(name, *self._head(xyz), *csr, *self._table(), _ffi.ptr(g), _ffi.ptr(ws), nbytes,
                  _ffi.ptr(dx), _ffi.stream())
        return dx


def acsf_values(layer, z, xyz, idx):
    """Flat ``(N, R*m)`` symmetry functions of a ragged batch (engine kernels; on the tape when xyz requires grad)."""
    from ...autograd import ACSF, needs_grad
    _ffi.require_device(xyz.values, idx.values)
    if xyz.values.dtype != torch.float32:
        raise TypeError("ACSF expects float32 coordinates, got %s" % xyz.values.dtype)
    if int(idx.values.shape[-1]) != (3 if isinstance(layer, ACSFG4) else 2):
        raise ValueError("%s expects index tuples of length %d" % (type(layer).__name__,
                                                                    3 if isinstance(layer, ACSFG4) else 2))
    plan = idx.index_plan(xyz)
    zv = z.values
    if zv.dtype != torch.int64:
        zv = zv.to(torch.int64)     # the reference casts the node numbers to the index dtype (acsf_conv.py:200)
    spec = AcsfSpec(layer, zv.contiguous(), plan)
    if needs_grad(xyz.values):
        return ACSF.apply(xyz.values, spec)
    return spec.forward(xyz.values)


class _ACSFBase(GraphBaseLayer):
    _max_atomic_number = _MAX_Z
    weight_gradients = True   # layers/base.py: the layer has no weights that train

    def _check_param_args(self, param_trainable, add_eps):
        if param_trainable:
            raise NotImplementedError("trainable ACSF parameters are not implemented (param_trainable=True)")
        if add_eps:
            raise NotImplementedError("ACSF with add_eps=True is not implemented")

    def call(self, inputs, mask=None, **kwargs):
        z, xyz, idx = self.assert_ragged_input_rank(inputs, mask=mask, ragged_rank=1)
        return xyz.with_values(acsf_values(self, z, xyz, idx))


class ACSFG2(_ACSFBase):
    r"""Radial symmetry functions :math:`G_i^2 = \sum_{j \neq i} e^{-\eta (r_{ij} - R_s)^2} f_c(r_{ij})`, one block of
    ``m`` functions per element of the neighbour (kgcnn/layers/conv/acsf_conv.py:16-224)."""

    def __init__(self, eta_rs_rc, element_mapping, add_eps=False, param_constraint=None, param_regularizer=None,
                 param_initializer="zeros", param_trainable=False, **kwargs):
        super().__init__(**kwargs)
        self._check_param_args(param_trainable, add_eps)
        self.eta_rs_rc = np.array(eta_rs_rc)
        assert len(self.eta_rs_rc.shape) in [3, 4], "Require `eta_rs_rc` of shape `(N, N, m, 3)` or `(N, m, 3)`"
        self.use_target_set = len(self.eta_rs_rc.shape) == 4
        self.num_relations = self.eta_rs_rc.shape[1] if self.use_target_set else self.eta_rs_rc.shape[0]
        self.num_functions = int(self.eta_rs_rc.shape[-2])
        self.num_centers = int(self.eta_rs_rc.shape[0]) if self.use_target_set else 0
        self.element_mapping = np.array(element_mapping, dtype="int")
        self.reverse_mapping = np.empty(self._max_atomic_number, dtype="int")
        self.reverse_mapping.fill(np.iinfo(self.reverse_mapping.dtype).max)
        for i, pos in enumerate(self.element_mapping):
            self.reverse_mapping[pos] = i
        self.add_eps = add_eps
        self.param_constraint, self.param_regularizer = param_constraint, param_regularizer
        self.param_initializer, self.param_trainable = param_initializer, param_trainable
        self._param_table = self.eta_rs_rc.astype(np.float32)

    @staticmethod
    def make_param_table(eta: list, rs: list, rc: float, elements: list, **kwargs):
        """Table for one cutoff: every (eta, rs) pair, rs-major, broadcast over the sorted elements."""
        eta_rs_rc = [(et, r_s, rc) for r_s in rs for et in eta]
        elements = np.sort(elements)
        params = np.broadcast_to(eta_rs_rc, (len(elements), len(eta_rs_rc), 3))
        return {"eta_rs_rc": params, "element_mapping": elements, **kwargs}

    def get_config(self):
        config = super().get_config()
        config.update({"eta_rs_rc": self.eta_rs_rc.tolist(), "element_mapping": self.element_mapping.tolist(),
                       "add_eps": self.add_eps, "param_constraint": self.param_constraint,
                       "param_regularizer": self.param_regularizer, "param_initializer": self.param_initializer,
                       "param_trainable": self.param_trainable})
        return config


class ACSFG4(_ACSFBase):
    r"""Angular symmetry functions :math:`G_i^4 = \sum_{j,k} 2^{1-\zeta} (1 + \lambda \cos\theta_{ijk})^\zeta
    e^{-\eta (r_{ij}^2 + r_{ik}^2 + r_{jk}^2)} f_{ij} f_{ik} f_{jk}`, one block per element pair of (j, k)
    (kgcnn/layers/conv/acsf_conv.py:227-510)."""

    def __init__(self, eta_zeta_lambda_rc, element_mapping, element_pair_mapping=None, add_eps=False,
                 keep_pair_order=False, multiplicity=None, param_initializer="zeros", param_regularizer=None,
                 param_constraint=None, param_trainable=False, **kwargs):
        super().__init__(**kwargs)
        self._check_param_args(param_trainable, add_eps)
        self.add_eps = add_eps
        self.multiplicity = multiplicity
        self.keep_pair_order = keep_pair_order
        self.eta_zeta_lambda_rc = np.array(eta_zeta_lambda_rc, dtype="float")
        assert len(self.eta_zeta_lambda_rc.shape) in [3, 4], "Require `eta_zeta_lambda_rc` rank 3 or 4."
        self.use_target_set = len(self.eta_zeta_lambda_rc.shape) == 4
        self.num_relations = self.eta_zeta_lambda_rc.shape[1] if self.use_target_set else \
            self.eta_zeta_lambda_rc.shape[0]
        self.num_functions = int(self.eta_zeta_lambda_rc.shape[-2])
        self.num_centers = int(self.eta_zeta_lambda_rc.shape[0]) if self.use_target_set else 0
        self.element_mapping = np.array(element_mapping, dtype="int")
        if element_pair_mapping is None:
            n = len(self.element_mapping)
            # entry a*n + b is (element b, element a), as the reference builds it (acsf_conv.py:314-320)
            pairs = np.stack([np.tile(self.element_mapping, n), np.repeat(self.element_mapping, n)], axis=-1)
            if not self.keep_pair_order:
                pairs = np.sort(pairs, axis=-1)
                first = np.unique(pairs, axis=0, return_index=True)[1]
                pairs = pairs[np.sort(first)]          # unordered pairs in order of first appearance
            self.element_pair_mapping = pairs
        else:
            self.element_pair_mapping = np.array(element_pair_mapping, dtype="int")
        assert len(self.element_pair_mapping.shape) == 2 and self.element_pair_mapping.shape[1] == 2
        assert self.element_pair_mapping.shape[0] == self.num_relations
        self.reverse_mapping = np.empty(self._max_atomic_number, dtype="int")
        self.reverse_mapping.fill(np.iinfo(self.reverse_mapping.dtype).max)
        for i, pos in enumerate(self.element_mapping):
            self.reverse_mapping[pos] = i
        self.reverse_pair_mapping = np.empty((self._max_atomic_number, self._max_atomic_number), dtype="int")
        self.reverse_pair_mapping.fill(np.iinfo(self.reverse_pair_mapping.dtype).max)
        for i, pos in enumerate(self.element_pair_mapping):
            self.reverse_pair_mapping[pos[0], pos[1]] = i
            if not self.keep_pair_order:
                self.reverse_pair_mapping[pos[1], pos[0]] = i
        self.param_constraint, self.param_regularizer = param_constraint, param_regularizer
        self.param_initializer, self.param_trainable = param_initializer, param_trainable
        self._param_table = self.eta_zeta_lambda_rc.astype(np.float32)

    @staticmethod
    def make_param_table(eta: list, zeta: list, lamda: list, rc: float, elements: list, **kwargs):
        """Table for one cutoff: every (eta, zeta, lambda) triple, eta-major, broadcast over the n(n+1)/2 element
        pairs of the sorted elements."""
        eta_zeta_lambda_rc = [[et, z, la, rc] for et in eta for z in zeta for la in lamda]
        elements = np.sort(elements)
        params = np.broadcast_to(
            eta_zeta_lambda_rc, (int(len(elements) * (len(elements) + 1) / 2), len(eta_zeta_lambda_rc), 4))
        return {"eta_zeta_lambda_rc": params, "element_mapping": elements, "element_pair_mapping": None, **kwargs}

    def get_config(self):
        config = super().get_config()
        config.update({"eta_zeta_lambda_rc": self.eta_zeta_lambda_rc, "add_eps": self.add_eps,
                       "element_mapping": self.element_mapping, "keep_pair_order": self.keep_pair_order,
                       "multiplicity": self.multiplicity, "element_pair_mapping": self.element_pair_mapping,
                       "param_trainable": self.param_trainable, "param_constraint": self.param_constraint,
                       "param_regularizer": self.param_regularizer, "param_initializer": self.param_initializer})
        return config


class ACSFConstNormalization(GraphBaseLayer):
    """``(x - mean) / std`` with constants (kgcnn/layers/conv/acsf_conv.py:513-546); the division is a multiplication by
    ``1 / std`` on the engine's broadcasting elementwise kernel."""

    weight_gradients = True

    def __init__(self, std=1.0, mean=0.0, **kwargs):
        super().__init__(**kwargs)
        self._np_std = np.array(std)
        self._np_mean = np.array(mean)

    def call(self, inputs, mask=None, **kwargs):
        def scale(x):
            width = int(x.shape[-1])
            mean = np.broadcast_to(np.asarray(self._np_mean, np.float32), (width,))
            inv = np.broadcast_to(1.0 / np.asarray(self._np_std, np.float32), (width,))
            m = torch.from_numpy(np.ascontiguousarray(mean).reshape(1, width)).to(x.device)
            s = torch.from_numpy(np.ascontiguousarray(inv).reshape(1, width)).to(x.device)
            return binary_values(_ffi.MP_MUL, binary_values(_ffi.MP_SUB, x, m), s)
        return self.map_values(scale, inputs)

    def get_config(self):
        config = super().get_config()
        config.update({"mean": self._np_mean.tolist(), "std": self._np_std.tolist()})
        return config
