"""DimeNet++ layers (mirror of kgcnn/layers/conv/dimenet_conv.py:13-463) on the HIP engine.

``SphericalBasisLayer`` runs ``mp_spherical_basis_f32`` (csrc/mp_dimenet.hip): the per-edge radial part and the
per-triplet product with ``Y_l0`` in two launches.  ``DimNetInteractionPPBlock`` runs its triplet step - gather of the
down-projected messages by angle column 1, the two bias-free ``W_sbf`` Dense layers on the spherical basis, the product
and the sum into angle column 0 (dimenet_conv.py:186-197) - as ONE launch, ``mp_dimenet_triplet_f32``, that keeps every
triplet-sized intermediate in registers.  The fused kernel serves ``int_emb_size`` 64, ``basis_emb_size`` 8 and up to 64
basis functions; other sizes take the reference's layer sequence on the existing engine kernels, as ``SchNetCFconv``
steps aside to its fallback.

Reverse rules (forces): ``autograd.SphericalBasis`` and ``autograd.DimeTriplet``, first order only.  The weights stay
frozen (``weight_gradients = False``): a weight that requires grad in grad mode raises ``NotImplementedError``.

The Bessel zeros and their normalisation (kgcnn/ops/polynom.py:201-245) are computed with NumPy when the layer is built:
the roots by bisection on the same float32-rounded brackets as the reference's ``brentq`` loop, rounded to float32 as
its ``zerosj`` array is, and the normaliser from the rounded zeros.
"""
import math

import numpy as np
import torch

from ... import _ffi
from ..base import GraphBaseLayer, Layer
from ..gather import GatherNodesOutgoing
from ..geom import angle_plan
from ..mlp import GraphMLP
from ..modules import Dense, LazyAdd, LazyMultiply
from ..pooling import PoolingLocalEdges


# ---------------------------------------------------------------------------------------------------- host tables
def _spherical_jn(x, n):
    """j_n(x) in float64 by upward recursion (adequate for the x > n where the zeros of j_n lie)."""
    x = np.asarray(x, dtype=np.float64)
    j0 = np.sin(x) / x
    if n == 0:
        return j0
    j1 = np.sin(x) / x ** 2 - np.cos(x) / x
    for i in range(1, n):
        j0, j1 = j1, (2 * i + 1) / x * j1 - j0
    return j1


def _bracketed_root(n, a, b, iters=200):
    """The zero of j_n in [a, b] (a sign change) by bisection to float64 resolution."""
    a, b = float(a), float(b)
    fa = _spherical_jn(a, n)
    for _ in range(iters):
        c = 0.5 * (a + b)
        if c == a or c == b:
            break
        fc = _spherical_jn(c, n)
        if (fc > 0) == (fa > 0):
            a, fa = c, fc
        else:
            b = c
    return 0.5 * (a + b)


def spherical_bessel_jn_zeros(n, k):
    """First ``k`` zeros of ``j_0 .. j_{n-1}``, shape (n, k) float32 (kgcnn/ops/polynom.py:201-225): the zeros of
    ``j_i`` are searched between consecutive (float32-rounded) zeros of ``j_{i-1}``, as in the reference."""
    zerosj = np.zeros((n, k), dtype="float32")
    zerosj[0] = np.arange(1, k + 1) * np.pi
    points = np.arange(1, k + n) * np.pi
    racines = np.zeros(k + n - 1, dtype="float32")
    for i in range(1, n):
        for j in range(k + n - 1 - i):
            racines[j] = _bracketed_root(i, points[j], points[j + 1])
        points = racines
        zerosj[i][:k] = racines[:k]
    return zerosj


def spherical_bessel_jn_normalization_prefactor(n, k, zeros=None):
    """``1 / sqrt(0.5 j_{l+1}(z_lk)^2)`` of the float32 zeros, shape (n, k) float64 (polynom.py:227-245)."""
    zeros = spherical_bessel_jn_zeros(n, k) if zeros is None else zeros
    out = np.zeros((n, k), dtype=np.float64)
    for order in range(n):
        z = zeros[order].astype(np.float64)
        out[order] = 1 / (0.5 * _spherical_jn(z, order + 1) ** 2) ** 0.5
    return out


def legendre_coefficients(num_spherical):
    """(L, L//2 + 1) coefficients of ``x^(l-2i)`` in ``P_l`` and the ``Y_l0`` prefactors ``sqrt((2l+1)/4pi)`` (L)
    (polynom.py:117-147)."""
    kl = num_spherical // 2 + 1
    coef = np.zeros((num_spherical, kl), dtype=np.float64)
    for l in range(num_spherical):
        for i in range(l // 2 + 1):
            coef[l, i] = (-1) ** i * math.factorial(2 * l - 2 * i) / math.factorial(l - i) / \
                math.factorial(l - 2 * i) / math.factorial(i) / 2 ** l
    ynorm = np.array([np.sqrt((2 * l + 1) / 4 / np.pi) for l in range(num_spherical)], dtype=np.float64)
    return coef, ynorm


class SphericalBasisSpec:
    """One SphericalBasisLayer call bound to an angle plan: ``forward`` (d, theta) -> (sbf, rbf_env) and ``grad``."""

    def __init__(self, layer, plan, device):
        self.plan, self.tables = plan, layer._device_tables(device)
        self.L, self.R = layer.num_spherical, layer.num_radial
        self.cutoff, self.exponent = float(layer.cutoff), int(layer.envelope_exponent)

    def forward(self, d, theta):
        d, theta = d.contiguous(), theta.contiguous()
        e, t, lr = self.plan.N, self.plan.M, self.L * self.R
        rbf_env = torch.empty((e, lr), dtype=torch.float32, device=d.device)
        sbf = torch.empty((t, lr), dtype=torch.float32, device=d.device)
        _ffi.call("mp_spherical_basis_f32", _ffi.ptr(d), e, _ffi.ptr(theta), _ffi.ptr(self.plan.cols), t,
                  _ffi.ptr(self.tables), self.L, self.R, self.cutoff, self.exponent, _ffi.ptr(rbf_env), _ffi.ptr(sbf),
                  _ffi.stream())
        return sbf, rbf_env

    def grad(self, d, theta, rbf_env, g, want_d=True, want_theta=True):
        e, t = self.plan.N, self.plan.M
        d_bar = torch.empty((e, 1), dtype=torch.float32, device=d.device) if want_d else None
        theta_bar = torch.empty((t, 1), dtype=torch.float32, device=d.device) if want_theta else None
        ptr1, perm1, _ = self.plan.csr(1)
        _ffi.call("mp_spherical_basis_grad_f32", _ffi.ptr(d), e, _ffi.ptr(theta), _ffi.ptr(self.plan.cols), t,
                  _ffi.ptr(ptr1), _ffi.ptr(perm1), _ffi.ptr(self.tables), self.L, self.R, self.cutoff, self.exponent,
                  _ffi.ptr(rbf_env), _ffi.ptr(g.contiguous()), _ffi.ptr(d_bar), _ffi.ptr(theta_bar), _ffi.stream())
        return d_bar, theta_bar


class SphericalBasisLayer(GraphBaseLayer):
    r"""Spherical basis of DimeNet (kgcnn/layers/conv/dimenet_conv.py:380-463): for angle pair ``t = (n, m)``,
    ``sbf[t, l*R + k] = env(d_m / c) norm[l,k] j_l(z_lk d_m / c) Y_l0(theta_t)``.  Inputs ``[distance (batch, [M], 1),
    angles (batch, [K], 1), angle_index (batch, [K], 2)]``; output ``(batch, [K], num_spherical * num_radial)``."""

    weight_gradients = True   # layers/base.py: the layer has no weights

    def __init__(self, num_spherical, num_radial, cutoff, envelope_exponent=5, **kwargs):
        super().__init__(**kwargs)
        assert num_radial <= 64
        if not 1 <= int(num_spherical) <= _ffi.MP_SBF_MAX_SPHERICAL or int(num_radial) < 1:
            raise ValueError("SphericalBasisLayer supports 1 <= num_spherical <= %d and num_radial >= 1, got %r, %r"
                             % (_ffi.MP_SBF_MAX_SPHERICAL, num_spherical, num_radial))
        if not (float(cutoff) > 0 and 1 <= int(envelope_exponent) <= 32):
            raise ValueError("SphericalBasisLayer needs cutoff > 0 and 1 <= envelope_exponent <= 32")
        self.num_radial = num_radial
        self.num_spherical = num_spherical
        self.cutoff = cutoff
        self.inv_cutoff = np.float32(1 / cutoff)
        self.envelope_exponent = envelope_exponent
        self.bessel_n_zeros = spherical_bessel_jn_zeros(num_spherical, num_radial)
        self.bessel_norm = spherical_bessel_jn_normalization_prefactor(num_spherical, num_radial,
                                                                       zeros=self.bessel_n_zeros)
        self.legendre, self.ynorm = legendre_coefficients(num_spherical)
        self._tables = None

    def host_tables(self):
        """The kernel's float32 table: zeros (L,R) | norm (L,R) | Legendre coefficients (L, L//2+1) | prefactors (L)."""
        return np.concatenate([self.bessel_n_zeros.ravel(), self.bessel_norm.astype(np.float32).ravel(),
                               self.legendre.astype(np.float32).ravel(),
                               self.ynorm.astype(np.float32)]).astype(np.float32)

    def _device_tables(self, device):
        if self._tables is None or self._tables.device != device:
            self.__dict__["_tables"] = torch.from_numpy(self.host_tables()).to(device)
        return self._tables

    def call(self, inputs, **kwargs):
        dist, angles, idx = self.assert_ragged_input_rank(list(inputs))
        d, a = dist.values, angles.values
        if d.dtype != torch.float32 or a.dtype != torch.float32 or int(d.shape[-1]) != 1 or int(a.shape[-1]) != 1:
            raise ValueError("SphericalBasisLayer expects float32 distances (batch, [M], 1) and angles (batch, [K], 1)")
        plan = angle_plan(idx, dist, self)
        if int(a.shape[0]) != plan.M:
            raise ValueError("SphericalBasisLayer: %d angles for %d angle pairs" % (int(a.shape[0]), plan.M))
        spec = SphericalBasisSpec(self, plan, d.device)
        from ...autograd import SphericalBasis, needs_grad
        if needs_grad(d, a):
            return angles.with_values(SphericalBasis.apply(d, a, spec))
        return angles.with_values(spec.forward(d, a)[0])

    def get_config(self):
        config = super().get_config()
        config.update({"num_radial": self.num_radial, "cutoff": self.cutoff,
                       "envelope_exponent": self.envelope_exponent, "num_spherical": self.num_spherical})
        return config


# ---------------------------------------------------------------------------------------------------- blocks
def _kernel_args(kernel_regularizer, bias_regularizer, activity_regularizer, kernel_constraint, bias_constraint,
                 kernel_initializer, bias_initializer):
    return {"kernel_regularizer": kernel_regularizer, "activity_regularizer": activity_regularizer,
            "bias_regularizer": bias_regularizer, "kernel_constraint": kernel_constraint,
            "bias_constraint": bias_constraint, "kernel_initializer": kernel_initializer,
            "bias_initializer": bias_initializer}


class ResidualLayer(GraphBaseLayer):
    """Residual layer of DimeNet++, ``x + dense_2(dense_1(x))`` (kgcnn/layers/conv/dimenet_conv.py:13-77)."""

    def __init__(self, units, use_bias=True, activation='kgcnn>swish', kernel_regularizer=None, bias_regularizer=None,
                 activity_regularizer=None, kernel_constraint=None, bias_constraint=None,
                 kernel_initializer='glorot_uniform', bias_initializer='zeros', **kwargs):
        super().__init__(**kwargs)
        dense_args = {"units": units, "activation": activation, "use_bias": use_bias}
        dense_args.update(_kernel_args(kernel_regularizer, bias_regularizer, activity_regularizer, kernel_constraint,
                                       bias_constraint, kernel_initializer, bias_initializer))
        self.dense_1 = Dense(**dense_args)
        self.dense_2 = Dense(**dense_args)
        self.add_end = LazyAdd()

    def build(self, input_shape):
        super().build(input_shape)
        self.dense_1.ensure_built(input_shape)
        self.dense_2.ensure_built(tuple(input_shape[:-1]) + (self.dense_1.units,))

    def call(self, inputs, **kwargs):
        x = self.dense_1(inputs, **kwargs)
        x = self.dense_2(x, **kwargs)
        return self.add_end([inputs, x], **kwargs)

    def get_config(self):
        config = super().get_config()
        conf_dense = self.dense_1.get_config()
        for x in ["kernel_regularizer", "activity_regularizer", "bias_regularizer", "kernel_constraint",
                  "bias_constraint", "kernel_initializer", "bias_initializer", "activation", "use_bias", "units"]:
            config.update({x: conf_dense[x]})
        return config


class TripletSpec:
    """The fused triplet step bound to an angle plan and the frozen ``W_sbf1`` (nsbf, 8) / ``W_sbf2`` (8, 64)."""

    def __init__(self, plan, w1, w2):
        self.plan, self.w1, self.w2 = plan, w1.detach(), w2.detach()
        self.nsbf, self.basis, self.units = int(w1.shape[0]), int(w1.shape[1]), int(w2.shape[1])

    def forward(self, xdown, sbf):
        ptr0, perm0, _ = self.plan.csr(0)
        out = torch.empty((self.plan.N, self.units), dtype=torch.float32, device=xdown.device)
        _ffi.call("mp_dimenet_triplet_f32", _ffi.ptr(xdown), self.plan.N, _ffi.ptr(sbf), self.nsbf,
                  _ffi.ptr(self.plan.cols), self.plan.M, _ffi.ptr(ptr0), _ffi.ptr(perm0), _ffi.ptr(self.w1), self.basis,
                  _ffi.ptr(self.w2), self.units, _ffi.ptr(out), _ffi.stream())
        return out

    def grad(self, xdown, sbf, g, want_x=True, want_s=True):
        ptr1, perm1, _ = self.plan.csr(1)
        x_bar = torch.empty_like(xdown) if want_x else None
        s_bar = torch.empty_like(sbf) if want_s else None
        if x_bar is None and s_bar is None:
            return None, None
        _ffi.call("mp_dimenet_triplet_grad_f32", _ffi.ptr(xdown), self.plan.N, _ffi.ptr(sbf), self.nsbf,
                  _ffi.ptr(self.plan.cols), self.plan.M, _ffi.ptr(ptr1), _ffi.ptr(perm1), _ffi.ptr(self.w1),
                  self.basis, _ffi.ptr(self.w2), self.units, _ffi.ptr(g.contiguous()), _ffi.ptr(x_bar),
                  _ffi.ptr(s_bar), _ffi.stream())
        return x_bar, s_bar


FUSED_TRIPLET_SIZES = {"int_emb_size": 64, "basis_emb_size": 8, "max_sbf": 64}   # csrc/mp_dimenet.hip


class DimNetInteractionPPBlock(GraphBaseLayer):
    """DimeNet++ interaction block (kgcnn/layers/conv/dimenet_conv.py:80-228).  Inputs ``[edges (batch, [M], F),
    rbf (batch, [M], R), sbf (batch, [K], L*R), angle_index (batch, [K], 2)]``; returns the updated edge embeddings.

    The triplet step is the fused ``mp_dimenet_triplet_f32`` when ``int_emb_size`` is 64, ``basis_emb_size`` 8, the
    spherical basis at most 64 wide and ``pooling_method`` "sum"; otherwise (or with ``use_fused_triplet = False``)
    the reference's GatherNodesOutgoing / Dense / LazyMultiply / PoolingLocalEdges sequence."""

    def __init__(self, emb_size, int_emb_size, basis_emb_size, num_before_skip, num_after_skip, use_bias=True,
                 pooling_method="sum", activation='kgcnn>swish', kernel_regularizer=None, bias_regularizer=None,
                 activity_regularizer=None, kernel_constraint=None, bias_constraint=None,
                 kernel_initializer="kgcnn>glorot_orthogonal", bias_initializer='zeros', **kwargs):
        super().__init__(**kwargs)
        self.use_bias = use_bias
        self.pooling_method = pooling_method
        self.emb_size = emb_size
        self.int_emb_size = int_emb_size
        self.basis_emb_size = basis_emb_size
        self.num_before_skip = num_before_skip
        self.num_after_skip = num_after_skip
        kernel_args = _kernel_args(kernel_regularizer, bias_regularizer, activity_regularizer, kernel_constraint,
                                   bias_constraint, kernel_initializer, bias_initializer)

        # Transformations of Bessel and spherical basis representations
        self.dense_rbf1 = Dense(basis_emb_size, use_bias=False, **kernel_args)
        self.dense_rbf2 = Dense(emb_size, use_bias=False, **kernel_args)
        self.dense_sbf1 = Dense(basis_emb_size, use_bias=False, **kernel_args)
        self.dense_sbf2 = Dense(int_emb_size, use_bias=False, **kernel_args)

        # Dense transformations of input messages
        self.dense_ji = Dense(emb_size, activation=activation, use_bias=True, **kernel_args)
        self.dense_kj = Dense(emb_size, activation=activation, use_bias=True, **kernel_args)

        # Embedding projections for interaction triplets
        self.down_projection = Dense(int_emb_size, activation=activation, use_bias=False, **kernel_args)
        self.up_projection = Dense(emb_size, activation=activation, use_bias=False, **kernel_args)

        # Residual layers before and after the skip connection
        self.layers_before_skip = [ResidualLayer(emb_size, activation=activation, use_bias=True, **kernel_args)
                                   for _ in range(num_before_skip)]
        self.final_before_skip = Dense(emb_size, activation=activation, use_bias=True, **kernel_args)
        self.layers_after_skip = [ResidualLayer(emb_size, activation=activation, use_bias=True, **kernel_args)
                                  for _ in range(num_after_skip)]

        self.lay_add1 = LazyAdd()
        self.lay_add2 = LazyAdd()
        self.lay_mult1 = LazyMultiply()
        self.lay_mult2 = LazyMultiply()
        self.lay_gather = GatherNodesOutgoing()
        self.lay_pool = PoolingLocalEdges(pooling_method=pooling_method)
        self.use_fused_triplet = True

    def build(self, input_shape):
        super().build(input_shape)
        x_shape, rbf_shape, sbf_shape = [tuple(s) for s in input_shape[:3]]
        lead = x_shape[:-1]
        self.dense_rbf1.ensure_built(rbf_shape)
        self.dense_rbf2.ensure_built(lead + (self.basis_emb_size,))
        self.dense_sbf1.ensure_built(sbf_shape)
        self.dense_sbf2.ensure_built(lead + (self.basis_emb_size,))
        for layer in (self.dense_ji, self.dense_kj, self.down_projection):
            layer.ensure_built(x_shape)
        self.up_projection.ensure_built(lead + (self.int_emb_size,))
        for layer in self.layers_before_skip + [self.final_before_skip] + self.layers_after_skip:
            layer.ensure_built(lead + (self.emb_size,))

    def fused_triplet(self, sbf_width):
        """True when the triplet step runs on ``mp_dimenet_triplet_f32`` for a spherical basis this wide."""
        s = FUSED_TRIPLET_SIZES
        return (self.use_fused_triplet and self.int_emb_size == s["int_emb_size"]
                and self.basis_emb_size == s["basis_emb_size"] and 1 <= sbf_width <= s["max_sbf"]
                and self.pooling_method == "sum")

    def triplet_step(self, x_kj, rbf, sbf, id_expand, **kwargs):
        """``sum_{t: A[t,0] = n} x_kj[A[t,1]] * ((sbf_t W_sbf1) W_sbf2)`` (dimenet_conv.py:186-197)."""
        if self.fused_triplet(int(sbf.values.shape[-1])):
            plan = angle_plan(id_expand, x_kj, self)
            if plan.N != int(rbf.values.shape[0]):
                raise ValueError("%s: %d edge rows for %d rbf rows" % (self.name, plan.N, int(rbf.values.shape[0])))
            spec = TripletSpec(plan, self.dense_sbf1.kernel, self.dense_sbf2.kernel)
            from ...autograd import DimeTriplet, needs_grad
            xv, sv = x_kj.values.contiguous(), sbf.values.contiguous()
            if needs_grad(xv, sv):
                return rbf.with_values(DimeTriplet.apply(xv, sv, spec))
            return rbf.with_values(spec.forward(xv, sv))
        x_kj = self.lay_gather([x_kj, id_expand], **kwargs)
        sbf = self.dense_sbf1(sbf, **kwargs)
        sbf = self.dense_sbf2(sbf, **kwargs)
        x_kj = self.lay_mult2([x_kj, sbf], **kwargs)
        return self.lay_pool([rbf, x_kj, id_expand], **kwargs)

    def call(self, inputs, **kwargs):
        x, rbf, sbf, id_expand = inputs

        # Initial transformation
        x_ji = self.dense_ji(x, **kwargs)
        x_kj = self.dense_kj(x, **kwargs)

        # Transform via Bessel basis
        rbf_t = self.dense_rbf1(rbf, **kwargs)
        rbf_t = self.dense_rbf2(rbf_t, **kwargs)
        x_kj = self.lay_mult1([x_kj, rbf_t], **kwargs)

        # Down-project, triplet step over the angle pairs, up-project
        x_kj = self.down_projection(x_kj, **kwargs)
        x_kj = self.triplet_step(x_kj, rbf_t, sbf, id_expand, **kwargs)
        x_kj = self.up_projection(x_kj, **kwargs)

        # Transformations before skip connection
        x2 = self.lay_add1([x_ji, x_kj], **kwargs)
        for layer in self.layers_before_skip:
            x2 = layer(x2, **kwargs)
        x2 = self.final_before_skip(x2, **kwargs)

        # Skip connection and transformations after it
        x = self.lay_add2([x, x2], **kwargs)
        for layer in self.layers_after_skip:
            x = layer(x, **kwargs)
        return x

    def get_config(self):
        config = super().get_config()
        config.update({"use_bias": self.use_bias, "pooling_method": self.pooling_method, "emb_size": self.emb_size,
                       "int_emb_size": self.int_emb_size, "basis_emb_size": self.basis_emb_size,
                       "num_before_skip": self.num_before_skip, "num_after_skip": self.num_after_skip})
        conf_dense = self.dense_ji.get_config()
        for x in ["kernel_regularizer", "activity_regularizer", "bias_regularizer", "kernel_constraint",
                  "bias_constraint", "kernel_initializer", "bias_initializer", "activation"]:
            config.update({x: conf_dense[x]})
        return config


class DimNetOutputBlock(GraphBaseLayer):
    """DimeNet++ output block (kgcnn/layers/conv/dimenet_conv.py:231-325): ``dense_rbf(rbf) * x`` summed into the
    receiving atoms, up-projection, ``num_dense`` Dense layers and a bias-free final Dense to ``num_targets``.  Inputs
    ``[nodes (batch, [N], F), edges (batch, [M], F), rbf (batch, [M], R), edge_index (batch, [M], 2)]``."""

    def __init__(self, emb_size, out_emb_size, num_dense, num_targets=12, use_bias=True,
                 output_kernel_initializer="zeros", kernel_initializer='kgcnn>glorot_orthogonal',
                 bias_initializer='zeros', activation='kgcnn>swish', kernel_regularizer=None, bias_regularizer=None,
                 activity_regularizer=None, kernel_constraint=None, bias_constraint=None, pooling_method="sum",
                 **kwargs):
        super().__init__(**kwargs)
        self.pooling_method = pooling_method
        self.emb_size = emb_size
        self.out_emb_size = out_emb_size
        self.num_dense = num_dense
        self.num_targets = num_targets
        self.use_bias = use_bias
        kernel_args = {"kernel_regularizer": kernel_regularizer, "activity_regularizer": activity_regularizer,
                       "kernel_constraint": kernel_constraint, "bias_initializer": bias_initializer,
                       "bias_regularizer": bias_regularizer, "bias_constraint": bias_constraint}
        self.dense_rbf = Dense(emb_size, use_bias=False, kernel_initializer=kernel_initializer, **kernel_args)
        self.up_projection = Dense(out_emb_size, use_bias=False, kernel_initializer=kernel_initializer, **kernel_args)
        self.dense_mlp = GraphMLP([out_emb_size] * num_dense, activation=activation,
                                  kernel_initializer=kernel_initializer, use_bias=use_bias, **kernel_args)
        self.dimnet_mult = LazyMultiply()
        self.pool = PoolingLocalEdges(pooling_method=self.pooling_method)
        self.dense_final = Dense(num_targets, use_bias=False, kernel_initializer=output_kernel_initializer,
                                 **kernel_args)

    def build(self, input_shape):
        super().build(input_shape)
        x_shape, rbf_shape = tuple(input_shape[1]), tuple(input_shape[2])
        lead = x_shape[:-1]
        self.dense_rbf.ensure_built(rbf_shape)
        self.up_projection.ensure_built(lead + (self.emb_size,))
        self.dense_mlp.ensure_built(lead + (self.out_emb_size,))
        self.dense_final.ensure_built(lead + (self.out_emb_size,))

    def call(self, inputs, **kwargs):
        n_atoms, x, rbf, idnb_i = inputs
        g = self.dense_rbf(rbf, **kwargs)
        x = self.dimnet_mult([g, x], **kwargs)
        x = self.pool([n_atoms, x, idnb_i], **kwargs)
        x = self.up_projection(x, **kwargs)
        x = self.dense_mlp(x, **kwargs)
        return self.dense_final(x, **kwargs)

    def get_config(self):
        config = super().get_config()
        conf_mlp = self.dense_mlp.get_config()
        for x in ["kernel_regularizer", "activity_regularizer", "bias_regularizer", "kernel_constraint",
                  "bias_constraint", "kernel_initializer", "bias_initializer", "activation"]:
            config.update({x: conf_mlp[x][0]})
        conf_dense_output = self.dense_final.get_config()
        config.update({"output_kernel_initializer": conf_dense_output["kernel_initializer"]})
        config.update({"pooling_method": self.pooling_method, "use_bias": self.use_bias})
        config.update({"emb_size": self.emb_size, "out_emb_size": self.out_emb_size, "num_dense": self.num_dense,
                       "num_targets": self.num_targets})
        return config


class EmbeddingDimeBlock(Layer):
    """Embedding of DimeNet++ (kgcnn/layers/conv/dimenet_conv.py:328-377): a table of shape ``(input_dim + 1,
    output_dim)`` created with the layer, rows gathered by the (cast) node numbers on ``mp_embedding_f32``."""

    def __init__(self, input_dim, output_dim, embeddings_initializer='uniform', embeddings_regularizer=None,
                 embeddings_constraint=None, **kwargs):
        super().__init__(**kwargs)
        self._supports_ragged_inputs = True
        self.output_dim = output_dim
        self.input_dim = input_dim
        self.embeddings_initializer = embeddings_initializer
        self.embeddings_regularizer = embeddings_regularizer
        self.embeddings_constraint = embeddings_constraint
        self.embeddings = self.add_weight("embeddings", (self.input_dim + 1, self.output_dim),
                                          self.embeddings_initializer)
        self.built = True

    def call(self, inputs, **kwargs):
        from ...ragged import RaggedTensor
        vals = inputs.values if isinstance(inputs, RaggedTensor) else inputs
        _ffi.require_device(vals)
        numbers = vals.to(torch.float32).contiguous()
        vocab, dim = int(self.embeddings.shape[0]), int(self.embeddings.shape[1])
        out = torch.empty(tuple(numbers.shape) + (dim,), dtype=torch.float32, device=vals.device)
        if numbers.numel():
            _ffi.call("mp_embedding_f32", _ffi.ptr(self.embeddings), vocab, dim, _ffi.ptr(numbers), numbers.numel(),
                      _ffi.ptr(out), None, _ffi.stream())
        return inputs.with_values(out) if isinstance(inputs, RaggedTensor) else out

    def get_config(self):
        config = super().get_config()
        config.update({"input_dim": self.input_dim, "output_dim": self.output_dim,
                       "embeddings_initializer": self.embeddings_initializer,
                       "embeddings_regularizer": self.embeddings_regularizer,
                       "embeddings_constraint": self.embeddings_constraint})
        return config
