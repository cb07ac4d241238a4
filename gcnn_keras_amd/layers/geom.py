"""Geometry pre-step layers of SchNet / PaiNN (mirror of the seven hot-path classes of kgcnn/layers/geom.py)."""
import numpy as np
import torch

from .. import _ffi
from ..ops.axis import get_positive_axis
from .base import GraphBaseLayer
from .gather import GatherNodesSelection
from .modules import LazyAdd, LazyMultiply, LazySubtract


class NodePosition(GraphBaseLayer):
    r"""Node positions for the two ends of every edge = ``GatherNodesSelection([0, 1])`` (kgcnn/layers/geom.py:14-73)."""

    weight_gradients = True   # layers/base.py: no weight of this layer is left off the tape

    def __init__(self, selection_index: list = None, **kwargs):
        super().__init__(**kwargs)
        if selection_index is None:
            selection_index = [0, 1]
        self.selection_index = selection_index
        self.layer_gather = GatherNodesSelection(self.selection_index)

    def call(self, inputs, **kwargs):
        return self.layer_gather(inputs, **kwargs)

    def get_config(self):
        config = super().get_config()
        config.update({"selection_index": self.selection_index})
        return config


def _rdc(values, axis_values):
    """View a values tensor as (R, D, C) with D the reduced axis."""
    shape = [int(s) for s in values.shape]
    r = 1
    for s in shape[:axis_values]:
        r *= s
    c = 1
    for s in shape[axis_values + 1:]:
        c *= s
    return r, shape[axis_values], c


def _lattice_shift_raw(pos, image, lattice, edge_splits):
    _ffi.require_device(pos, image, lattice, edge_splits)
    p, im, lat = pos.contiguous(), image.contiguous(), lattice.contiguous()
    m, g = int(p.shape[0]), int(lat.shape[0])
    out = torch.empty_like(p)
    _ffi.call("mp_lattice_shift_f32", _ffi.ptr(p), _ffi.ptr(im), _ffi.ptr(lat), _ffi.ptr(edge_splits), g, m,
              _ffi.ptr(out), _ffi.stream())
    return out


class ShiftPeriodicLattice(GraphBaseLayer):
    r"""``x + n_1 a_1 + n_2 a_2 + n_3 a_3`` for positions ``x`` ``(batch, [M], 3)``, image indices ``n``
    ``(batch, [M], 3)`` int64 and one lattice matrix ``(batch, 3, 3)`` per graph, lattice vectors in rows
    (kgcnn/layers/geom.py:76-123).  The sum runs in the reference's order, ``x + ((n_1 a_1 + n_2 a_2) + n_3 a_3)``,
    without contraction.  The output carries the partition of the image tensor.  Linear in the position; a lattice that
    requires grad raises (stress is not implemented)."""

    weight_gradients = True   # layers/base.py: no weight of this layer is left off the tape

    def call(self, inputs, **kwargs):
        from ..ragged import RaggedTensor
        if len(inputs) != 3:
            raise ValueError("ShiftPeriodicLattice expects [position, edge_image, lattice]")
        x, ei, lattice = inputs
        if not isinstance(x, RaggedTensor) or not isinstance(ei, RaggedTensor):
            raise TypeError("ShiftPeriodicLattice expects ragged positions and ragged image indices")
        if isinstance(lattice, RaggedTensor) or not torch.is_tensor(lattice):
            raise TypeError("ShiftPeriodicLattice expects the lattice as a dense tensor of shape (batch, 3, 3)")
        if ei.values.dtype != torch.int64:
            raise TypeError("edge_image must be int64, got %s" % ei.values.dtype)
        if x.values.dtype != torch.float32 or lattice.dtype != torch.float32:
            raise TypeError("ShiftPeriodicLattice expects float32 positions and lattice")
        if tuple(lattice.shape) != (ei.nrows(), 3, 3):
            raise ValueError("lattice must have shape (%d, 3, 3), got %s" % (ei.nrows(), tuple(lattice.shape)))
        if tuple(x.values.shape) != tuple(ei.values.shape) or x.values.dim() != 2 or int(x.values.shape[1]) != 3:
            raise ValueError("positions %s and images %s must both be (batch, [M], 3)"
                             % (tuple(x.values.shape), tuple(ei.values.shape)))
        if lattice.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("gradients with respect to the lattice (stress) are not implemented")
        from ..autograd import LatticeShift, needs_grad
        if needs_grad(x.values):
            return ei.with_values(LatticeShift.apply(x.values, ei.values, lattice, ei.row_splits))
        return ei.with_values(_lattice_shift_raw(x.values, ei.values, lattice, ei.row_splits))


class DisplacementVectorsUnitCell(GraphBaseLayer):
    r"""``f_i - (f_j + m_ij)`` for fractional coordinates ``f`` ``(batch, [N], 3)``, edge indices ``(batch, [M], 2)`` and
    cell translations ``m`` ``(batch, [M], 3)`` (kgcnn/layers/geom.py:964-1008): gather, add, subtract, as the
    reference composes it.  ``cell_translations`` is float32; an int64 tensor (``range_image`` of ``SetRangePeriodic``)
    is cast."""

    weight_gradients = True   # layers/base.py: the layer has no weights

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.gather_node_positions = NodePosition()
        self.lazy_add = LazyAdd()
        self.lazy_sub = LazySubtract()

    def call(self, inputs, **kwargs):
        frac_coords, edge_indices, cell_translations = inputs[0], inputs[1], inputs[2]
        if cell_translations.values.dtype == torch.int64:
            cell_translations = cell_translations.with_values(cell_translations.values.to(torch.float32))
        in_frac_coords, out_frac_coords = self.gather_node_positions([frac_coords, edge_indices], **kwargs)
        out_frac_coords = self.lazy_add([out_frac_coords, cell_translations], **kwargs)
        return self.lazy_sub([in_frac_coords, out_frac_coords], **kwargs)


def _frac_to_real_raw(frac, lattice, row_splits, transposed=False):
    _ffi.require_device(frac, lattice, row_splits)
    f, lat = frac.contiguous(), lattice.contiguous()
    out = torch.empty_like(f)
    _ffi.call("mp_frac_to_real_f32", _ffi.ptr(f), _ffi.ptr(lat), _ffi.ptr(row_splits), int(lat.shape[0]),
              int(f.shape[0]), 1 if transposed else 0, _ffi.ptr(out), _ffi.stream())
    return out


class FracToRealCoordinates(GraphBaseLayer):
    r"""Real-space from fractional coordinates ``(batch, [N], 3)`` and one lattice matrix ``(batch, 3, 3)`` per graph
    (kgcnn/layers/geom.py:1012-1052) on ``mp_frac_to_real_f32``.  The reference's einsum is ``'ij,ikj->ik'``:
    ``r_k = sum_j f_j A[k][j]``, that is :math:`\mathbf{A} \vec{f}` - NOT the :math:`\vec{f} \mathbf{A}` with lattice
    vectors in rows that its docstring promises.  The code is mirrored: a lattice in the row convention (pymatgen,
    ``SetRangePeriodic``) has to be passed **transposed**.  Linear in the coordinates (the reverse is the transposed
    product, differentiable any number of times); a lattice that requires grad raises."""

    weight_gradients = True   # layers/base.py: the layer has no weights

    def call(self, inputs, **kwargs):
        from ..ragged import RaggedTensor
        if len(inputs) != 2:
            raise ValueError("FracToRealCoordinates expects [frac_coordinates, lattice_matrix]")
        frac, lattice = self.assert_ragged_input_rank(inputs[0], ragged_rank=1), inputs[1]
        if isinstance(lattice, RaggedTensor) or not torch.is_tensor(lattice):
            raise TypeError("FracToRealCoordinates expects the lattice as a dense tensor of shape (batch, 3, 3)")
        if frac.values.dtype != torch.float32 or lattice.dtype != torch.float32:
            raise TypeError("FracToRealCoordinates expects float32 coordinates and lattice")
        if tuple(lattice.shape) != (frac.nrows(), 3, 3):
            raise ValueError("lattice must have shape (%d, 3, 3), got %s" % (frac.nrows(), tuple(lattice.shape)))
        if frac.values.dim() != 2 or int(frac.values.shape[1]) != 3:
            raise ValueError("fractional coordinates must be (batch, [N], 3), got %s" % (tuple(frac.values.shape),))
        if lattice.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("gradients with respect to the lattice (stress) are not implemented")
        from ..autograd import FracToReal, needs_grad
        if needs_grad(frac.values):
            return frac.with_values(FracToReal.apply(frac.values, lattice, frac.row_splits, False))
        return frac.with_values(_frac_to_real_raw(frac.values, lattice, frac.row_splits))


class EuclideanNorm(GraphBaseLayer):
    r"""``sqrt(relu(sum_axis x^2))`` with optional eps / inversion (kgcnn/layers/geom.py:127-214)."""

    weight_gradients = True   # layers/base.py: no weight of this layer is left off the tape

    def __init__(self, axis: int = -1, keepdims: bool = False, invert_norm: bool = False, add_eps: bool = False,
                 no_nan: bool = True, square_norm: bool = False, **kwargs):
        super().__init__(**kwargs)
        self.axis = axis
        self.keepdims = keepdims
        self.invert_norm = invert_norm
        self.square_norm = square_norm
        self.add_eps = add_eps
        self.no_nan = no_nan

    def build(self, input_shape):
        super().build(input_shape)
        self.axis = get_positive_axis(self.axis, len(input_shape))

    @staticmethod
    def _compute_euclidean_norm(inputs, axis: int = -1, keepdims: bool = False, invert_norm: bool = False,
                                add_eps: bool = False, no_nan: bool = True, square_norm: bool = False):
        _ffi.require_device(inputs)
        x = inputs.contiguous()
        ax = axis if axis >= 0 else axis + x.dim()
        r, d, c = _rdc(x, ax)
        shape = list(x.shape)
        out_shape = shape[:ax] + ([1] if keepdims else []) + shape[ax + 1:]
        out = torch.empty(out_shape, dtype=torch.float32, device=x.device)
        flags = (1 if invert_norm else 0) | (2 if add_eps else 0) | (4 if no_nan else 0) | (8 if square_norm else 0)
        from ..autograd import EuclideanNorm as NormFn, needs_grad
        if needs_grad(inputs):
            return NormFn.apply(inputs, r, d, c, flags, tuple(out_shape))
        _ffi.call("mp_euclidean_norm_f32", _ffi.ptr(x), r, d, c, flags, _ffi.ptr(out), _ffi.stream())
        return out

    def call(self, inputs, **kwargs):
        return self.map_values(self._compute_euclidean_norm, inputs, axis=self.axis, keepdims=self.keepdims,
                               invert_norm=self.invert_norm, add_eps=self.add_eps, no_nan=self.no_nan,
                               square_norm=self.square_norm)

    def get_config(self):
        config = super().get_config()
        config.update({"axis": self.axis, "keepdims": self.keepdims, "invert_norm": self.invert_norm,
                       "add_eps": self.add_eps, "no_nan": self.no_nan, "square_norm": self.square_norm})
        return config


class ScalarProduct(GraphBaseLayer):
    r"""``sum_axis a*b`` (kgcnn/layers/geom.py:218-281)."""

    weight_gradients = True   # layers/base.py: no weight of this layer is left off the tape

    def __init__(self, axis=-1, **kwargs):
        super().__init__(**kwargs)
        self.axis = axis

    def build(self, input_shape):
        super().build(input_shape)
        axis = get_positive_axis(self.axis, len(input_shape[0]))
        axis2 = get_positive_axis(self.axis, len(input_shape[1]))
        assert axis2 == axis, "Axis parameter must match on the two input vectors for scalar product."
        self.axis = axis

    @staticmethod
    def _scalar_product(inputs: list, axis: int, **kwargs):
        from ..autograd import ScalarProduct as ProdFn, needs_grad
        if needs_grad(inputs[0], inputs[1]):
            return ProdFn.apply(inputs[0], inputs[1], axis)
        a, b = inputs[0].contiguous(), inputs[1].contiguous()
        _ffi.require_device(a, b)
        r, d, c = _rdc(a, axis)
        shape = list(a.shape)
        out = torch.empty(shape[:axis] + shape[axis + 1:], dtype=torch.float32, device=a.device)
        _ffi.call("mp_scalar_product_f32", _ffi.ptr(a), _ffi.ptr(b), r, d, c, _ffi.ptr(out), _ffi.stream())
        return out

    def call(self, inputs, **kwargs):
        return self.map_values(self._scalar_product, inputs, axis=self.axis)

    def get_config(self):
        config = super().get_config()
        config.update({"axis": self.axis})
        return config


class NodeDistanceEuclidean(GraphBaseLayer):
    r"""``||x_1 - x_2||`` with kept last axis, shape ``(batch, [M], 1)`` (kgcnn/layers/geom.py:285-327)."""

    weight_gradients = True   # layers/base.py: no weight of this layer is left off the tape

    def __init__(self, add_eps: bool = False, no_nan: bool = True, **kwargs):
        super().__init__(**kwargs)
        self.layer_subtract = LazySubtract()
        self.layer_euclidean_norm = EuclideanNorm(axis=2, keepdims=True, add_eps=add_eps, no_nan=no_nan)

    def call(self, inputs, **kwargs):
        diff = self.layer_subtract(inputs)
        return self.layer_euclidean_norm(diff)

    def get_config(self):
        config = super().get_config()
        conf_norm = self.layer_euclidean_norm.get_config()
        config.update({"add_eps": conf_norm["add_eps"], "no_nan": conf_norm["no_nan"]})
        return config


class EdgeDirectionNormalized(GraphBaseLayer):
    r"""``(r_i - r_j) / ||r_i - r_j||`` with ``divide_no_nan`` (kgcnn/layers/geom.py:331-378)."""

    weight_gradients = True   # layers/base.py: no weight of this layer is left off the tape

    def __init__(self, add_eps: bool = False, no_nan: bool = True, **kwargs):
        super().__init__(**kwargs)
        self.layer_subtract = LazySubtract()
        self.layer_euclidean_norm = EuclideanNorm(axis=2, keepdims=True, invert_norm=True, add_eps=add_eps,
                                                  no_nan=no_nan)
        self.layer_multiply = LazyMultiply()

    def call(self, inputs, **kwargs):
        diff = self.layer_subtract(inputs)
        norm = self.layer_euclidean_norm(diff)
        return self.layer_multiply([diff, norm])

    def get_config(self):
        config = super().get_config()
        conf_norm = self.layer_euclidean_norm.get_config()
        config.update({"add_eps": conf_norm["add_eps"], "no_nan": conf_norm["no_nan"]})
        return config


class GaussBasisLayer(GraphBaseLayer):
    r"""Gaussian radial basis ``exp(-gamma (d - offset - mu_k)^2)``, ``mu_k = k / bins * distance``,
    ``gamma = 1 / (2 sigma^2)`` (kgcnn/layers/geom.py:514-592)."""

    weight_gradients = True   # layers/base.py: no weight of this layer is left off the tape

    def __init__(self, bins: int = 20, distance: float = 4.0, sigma: float = 0.4, offset: float = 0.0, **kwargs):
        super().__init__(**kwargs)
        self.bins = int(bins)
        self.distance = float(distance)
        self.offset = float(offset)
        self.sigma = float(sigma)
        self.gamma = 1 / sigma / sigma / 2

    def _compute_gauss_basis(self, inputs):
        _ffi.require_device(inputs)
        d = inputs.contiguous()
        if int(d.shape[-1]) != 1:
            raise ValueError("GaussBasisLayer expects distances of shape (batch, [K], 1)")
        from ..autograd import GaussBasis as GaussFn, needs_grad
        if needs_grad(inputs):
            return GaussFn.apply(inputs, self.bins, self.distance, self.sigma, self.offset)
        m = d.numel()
        out = torch.empty(tuple(d.shape[:-1]) + (self.bins,), dtype=torch.float32, device=d.device)
        _ffi.call("mp_gauss_basis_f32", _ffi.ptr(d), m, self.bins, self.distance, self.sigma, self.offset,
                  _ffi.ptr(out), _ffi.stream())
        return out

    def call(self, inputs, **kwargs):
        return self.map_values(self._compute_gauss_basis, inputs)

    def get_config(self):
        config = super().get_config()
        config.update({"bins": self.bins, "distance": self.distance, "offset": self.offset, "sigma": self.sigma})
        return config


class BesselBasisLayer(GraphBaseLayer):
    r"""Bessel radial basis with polynomial envelope (kgcnn/layers/geom.py:717-805): ``env(d/c) sin(f_k d/c)``,
    trainable ``frequencies`` initialised to ``pi * (1..num_radial)``, envelope zero for ``d/c >= 1``."""

    def __init__(self, num_radial: int, cutoff: float, envelope_exponent: int = 5, envelope_type: str = "poly",
                 **kwargs):
        super().__init__(**kwargs)
        self.num_radial = num_radial
        self.cutoff = cutoff
        self.envelope_exponent = envelope_exponent
        self.envelope_type = str(envelope_type)
        if self.envelope_type not in ["poly"]:
            raise ValueError("Unknown envelope type '%s' in `BesselBasisLayer`." % self.envelope_type)
        self.frequencies = self.add_weight(
            "frequencies", (self.num_radial,),
            initializer=lambda shape: np.pi * np.arange(1, shape[0] + 1, dtype=np.float32))

    def expand_bessel_basis(self, inputs):
        _ffi.require_device(inputs)
        d = inputs.contiguous()
        if int(d.shape[-1]) != 1:
            raise ValueError("BesselBasisLayer expects distances of shape (batch, [K], 1)")
        from ..autograd import BesselBasis as BesselFn, needs_grad
        if needs_grad(inputs):
            return BesselFn.apply(inputs, self.frequencies, self.num_radial, float(self.cutoff),
                                  int(self.envelope_exponent))
        out = torch.empty(tuple(d.shape[:-1]) + (self.num_radial,), dtype=torch.float32, device=d.device)
        _ffi.call("mp_bessel_basis_f32", _ffi.ptr(d), d.numel(), _ffi.ptr(self.frequencies), self.num_radial,
                  float(self.cutoff), int(self.envelope_exponent), _ffi.ptr(out), _ffi.stream())
        return out

    def call(self, inputs, **kwargs):
        return self.map_values(self.expand_bessel_basis, inputs)

    def get_config(self):
        config = super().get_config()
        config.update({"num_radial": self.num_radial, "cutoff": self.cutoff,
                       "envelope_exponent": self.envelope_exponent, "envelope_type": self.envelope_type})
        return config


class CosCutOffEnvelope(GraphBaseLayer):
    r"""``0.5 (cos(pi d / R_c) + 1)`` on clipped distances; ``cutoff=None`` means 1e8 (kgcnn/layers/geom.py:809-856)."""

    weight_gradients = True   # layers/base.py: no weight of this layer is left off the tape

    def __init__(self, cutoff, **kwargs):
        super().__init__(**kwargs)
        self.cutoff = float(np.abs(cutoff)) if cutoff is not None else 1e8

    def _compute_cutoff_envelope(self, inputs):
        _ffi.require_device(inputs)
        from ..autograd import CosCutoff as CosFn, needs_grad
        if needs_grad(inputs):
            return CosFn.apply(inputs, float(self.cutoff))
        d = inputs.contiguous()
        out = torch.empty_like(d)
        _ffi.call("mp_cos_cutoff_f32", _ffi.ptr(d), d.numel(), float(self.cutoff), _ffi.ptr(out), _ffi.stream())
        return out

    def call(self, inputs, **kwargs):
        return self.map_values(self._compute_cutoff_envelope, inputs)

    def get_config(self):
        config = super().get_config()
        config.update({"cutoff": self.cutoff})
        return config


def vector_angle_raw(v1, v2):
    """theta (T, 1) = atan2(|v1 x v2|, v1 . v2) of two contiguous (T, 3) tensors (``mp_vector_angle_f32``)."""
    t = int(v1.shape[0])
    out = torch.empty((t, 1), dtype=torch.float32, device=v1.device)
    if t:
        _ffi.call("mp_vector_angle_f32", _ffi.ptr(v1), _ffi.ptr(v2), t, _ffi.ptr(out), _ffi.stream())
    return out


class VectorAngle(GraphBaseLayer):
    r"""Angle between two vectors, :math:`\theta = \tan^{-1}(|\vec{v}_1 \times \vec{v}_2| / \vec{v}_1 \cdot \vec{v}_2)`
    (kgcnn/layers/geom.py:382-446) on ``mp_vector_angle_f32``; output ``(batch, [M], 1)``.  At collinear vectors the
    reverse gives a zero gradient where the reference's ``tf.norm`` gradient is NaN."""

    weight_gradients = True   # layers/base.py: the layer has no weights

    @staticmethod
    def _compute_vector_angle(inputs: list):
        v1, v2 = inputs[0], inputs[1]
        _ffi.require_device(v1, v2)
        if tuple(v1.shape) != tuple(v2.shape) or v1.dim() != 2 or int(v1.shape[-1]) != 3:
            raise ValueError("VectorAngle expects two (batch, [M], 3) tensors, got %s and %s"
                             % (tuple(v1.shape), tuple(v2.shape)))
        from ..autograd import VectorAngle as AngleFn, needs_grad
        if needs_grad(v1, v2):
            return AngleFn.apply(v1, v2)
        return vector_angle_raw(v1.contiguous(), v2.contiguous())

    def call(self, inputs, **kwargs):
        return self.map_values(self._compute_vector_angle, list(inputs))


class EdgeAngleSpec:
    """One EdgeAngle call bound to an angle index plan against the edges: ``forward`` (E, 3) -> (T, 1) and ``grad``."""

    def __init__(self, plan, scale):
        self.plan, self.scale = plan, scale

    def forward(self, v):
        out = torch.empty((self.plan.M, 1), dtype=torch.float32, device=v.device)
        _ffi.call("mp_edge_angle_f32", _ffi.ptr(v), self.plan.N, _ffi.ptr(self.plan.cols), self.plan.M,
                  _ffi.ptr(self.scale), _ffi.ptr(out), _ffi.stream())
        return out

    def grad(self, v, g):
        ws, nbytes = _ffi.float_workspace("mp_edge_angle_grad_ws_bytes", self.plan.M, device=v.device)
        v_bar = torch.empty_like(v)
        ptr0, perm0, _ = self.plan.csr(0)
        ptr1, perm1, _ = self.plan.csr(1)
        _ffi.call("mp_edge_angle_grad_f32", _ffi.ptr(v), self.plan.N, _ffi.ptr(self.plan.cols), self.plan.M,
                  _ffi.ptr(ptr0), _ffi.ptr(perm0), _ffi.ptr(ptr1), _ffi.ptr(perm1), _ffi.ptr(self.scale),
                  _ffi.ptr(g.contiguous()), _ffi.ptr(ws), nbytes, _ffi.ptr(v_bar), _ffi.stream())
        return v_bar


def angle_plan(idx, edges, layer):
    """Index plan of an angle list ``(batch, [T], 2)`` against the edge partition of ``edges``; out-of-range pairs raise
    ``IndexError`` (the DimeNet++ kernels read both edges of every pair)."""
    _ffi.require_device(edges.values, idx.values)
    if idx.values.dim() != 2 or int(idx.values.shape[-1]) != 2:
        raise ValueError("%s expects angle indices of shape (batch, [T], 2)" % layer.name)
    plan = idx.index_plan(edges)
    plan.validate()
    return plan


class EdgeAngle(GraphBaseLayer):
    r"""Angle between the vectors of the two edges of every angle pair ``(n, m)`` (kgcnn/layers/geom.py:450-510): the
    reference's ``GatherNodesSelection([0, 1])`` + ``VectorAngle`` as one kernel, ``mp_edge_angle_f32``.
    ``vector_scale``: two scales (scalars or 3-vectors) for the vectors of ``n`` and ``m``.  Output
    ``(batch, [T], 1)``."""

    weight_gradients = True   # layers/base.py: the layer has no weights

    def __init__(self, vector_scale: list = None, **kwargs):
        super().__init__(**kwargs)
        self.vector_scale = vector_scale
        if vector_scale:
            assert len(vector_scale) == 2, "Need scale for both vectors to compute angle."
        self._scale_host = None
        if vector_scale:
            self._scale_host = np.concatenate([np.broadcast_to(np.asarray(s, dtype=np.float32), (3,))
                                               for s in vector_scale]).astype(np.float32)
        self._scale_dev = None

    def _scale(self, device):
        if self._scale_host is None:
            return None
        if self._scale_dev is None or self._scale_dev.device != device:
            self._scale_dev = torch.from_numpy(self._scale_host.copy()).to(device)
        return self._scale_dev

    def call(self, inputs, **kwargs):
        vec, idx = self.assert_ragged_input_rank(list(inputs))
        v = vec.values
        if v.dtype != torch.float32 or v.dim() != 2 or int(v.shape[-1]) != 3:
            raise ValueError("EdgeAngle expects float32 edge vectors of shape (batch, [M], 3)")
        spec = EdgeAngleSpec(angle_plan(idx, vec, self), self._scale(v.device))
        from ..autograd import EdgeAngle as AngleFn, needs_grad
        if needs_grad(v):
            return idx.with_values(AngleFn.apply(v, spec))
        return idx.with_values(spec.forward(v.contiguous()))

    def get_config(self):
        config = super().get_config()
        config.update({"vector_scale": self.vector_scale})
        return config


def position_encoding_scales(dim_half, wave_length_min, num_mult):
    """``2 pi exp(-log(num_mult) i / (dim_half - 1) - log(wave_length_min))`` (dim_half,), every step rounded to float32
    as the reference's float32 graph builds it (kgcnn/layers/geom.py:677-681)."""
    steps = np.arange(dim_half, dtype=np.float32) / np.float32(dim_half - 1)
    log_num, log_wave = np.float32(-np.log(num_mult)), np.float32(-np.log(wave_length_min))
    freq = np.exp((log_num * steps + log_wave).astype(np.float32)).astype(np.float32)
    return (freq * np.float32(np.pi * 2.0)).astype(np.float32)


def position_encoding_raw(x, scales, interleave):
    """(M, 2K) encoding of contiguous x (M, 1) on ``mp_position_encoding_f32``."""
    m, k = int(x.shape[0]), int(scales.shape[0])
    out = torch.empty((m, 2 * k), dtype=torch.float32, device=x.device)
    _ffi.call("mp_position_encoding_f32", _ffi.ptr(x), m, _ffi.ptr(scales), k, 1 if interleave else 0, _ffi.ptr(out),
              _ffi.stream())
    return out


class PositionEncodingBasisLayer(GraphBaseLayer):
    r"""Positional (Fourier) encoding of a distance (kgcnn/layers/geom.py:596-713): ``[sin(x s_k) | cos(x s_k)]`` with
    ``s_k = 2 pi / (wave_length_min num_mult^(k / (dim_half - 1)))``, or sin and cos interleaved per ``k``
    (``interleave_sin_cos``), on ``mp_position_encoding_f32``; input ``(batch, [K], 1)``, output ``(batch, [K], 2
    dim_half)``.  ``include_frequencies=True`` is a ``TypeError`` inside the reference (``tf.concat(..., dim=-1)``) and
    raises ``NotImplementedError`` here."""

    weight_gradients = True   # layers/base.py: the layer has no weights

    def __init__(self, dim_half: int = 10, wave_length_min: float = 1, num_mult=100, include_frequencies: bool = False,
                 interleave_sin_cos: bool = False, **kwargs):
        super().__init__(**kwargs)
        self.dim_half = dim_half
        self.num_mult = num_mult
        self.wave_length_min = wave_length_min
        self.include_frequencies = include_frequencies
        self.interleave_sin_cos = interleave_sin_cos
        if self.num_mult <= 1:
            raise ValueError("`num_mult` must be >1. Reduce `wave_length_min` if necessary.")
        if self.dim_half <= 1:
            raise ValueError("`dim_half` must be > 1.")
        if self.include_frequencies:
            raise NotImplementedError("PositionEncodingBasisLayer(include_frequencies=True) fails in the reference "
                                      "(tf.concat(..., dim=-1)) and is not implemented")
        self.scales_host = position_encoding_scales(int(dim_half), wave_length_min, num_mult)
        self._scales = None

    def scales(self, device):
        if self._scales is None or self._scales.device != device:
            self.__dict__["_scales"] = torch.from_numpy(self.scales_host.copy()).to(device)
        return self._scales

    def _compute_fourier_encoding(self, inputs):
        _ffi.require_device(inputs)
        if inputs.dtype != torch.float32 or inputs.dim() != 2 or int(inputs.shape[-1]) != 1:
            raise ValueError("PositionEncodingBasisLayer expects float32 distances of shape (batch, [K], 1)")
        scales = self.scales(inputs.device)
        from ..autograd import PositionEncoding, needs_grad
        if needs_grad(inputs):
            return PositionEncoding.apply(inputs, scales, bool(self.interleave_sin_cos))
        return position_encoding_raw(inputs.contiguous(), scales, self.interleave_sin_cos)

    def call(self, inputs, **kwargs):
        return self.map_values(self._compute_fourier_encoding, inputs)

    def get_config(self):
        config = super().get_config()
        config.update({"dim_half": self.dim_half, "wave_length_min": self.wave_length_min, "num_mult": self.num_mult,
                       "include_frequencies": self.include_frequencies, "interleave_sin_cos": self.interleave_sin_cos})
        return config
