"""The relational message blocks of RGCN (kgcnn/literature/RGCN.py:96-103; Schlichtkrull et al. 2017) and GNNFilm
(kgcnn/literature/GNNFilm.py:93-102; Brockschmidt 2019) and their fused route on csrc/mp_rgcn.hip.  The reference spells
both blocks inline in ``make_model`` (its ``rgcn_conv.py`` is empty); here each is a layer.

``RGCNStep``: ``n' = act(sum_{e -> i} w_e RelationalDense(n_j, rel_e) + Dense(n_i))``.
``GNNFilmStep``: ``n' = act(sum_{e -> i} [gamma(n_i, rel_e) * RelationalDense(n_j, rel_e) + beta(n_i, rel_e)])`` with
``gamma`` and ``beta`` two ``RelationalDense`` on the RECEIVER's features.  Each has two routes:

* the *layer sequence*, the reference's ops on the engine's layers (``GatherNodesOutgoing`` / ``GatherNodesSelection``,
  ``Dense``, ``RelationalDense``, ``LazyMultiply``, ``LazyAdd``, ``PoolingLocalMessages``, ``Activation``): every
  configuration, every call with keyword arguments and every tape (all training);
* the *fused route*, one launch of ``mp_relational_conv_f32`` per block: the sum over a receiver's edges is taken in front
  of the per-relation product, which a linear message ``RelationalDense`` allows; FiLM's gamma and beta depend on
  (receiver, relation) only.  Nothing edge-sized is written.  With ``num_bases`` / ``num_blocks`` the effective kernels
  are assembled once per call (``DecomposedRelationalDense.effective_kernel``) and passed in.

Served sizes (``fused_relational_supported``, decided in ``build``): node width and units each in {32, 64, 128},
``1 <= num_relations <= 64``, a linear message ``RelationalDense`` (bias on or off), edge weights of width 1, every
activation among the engine's codes, float32, sum pooling into index column 0.  The fused route is forward-only: in grad
mode it steps aside when an input or a weight requires grad, and so do ``use_fused_relational = False`` and keyword
arguments.  Edge lists that are not receiver-sorted go through the plan's CSR permutation.

Every ``RelationalDense`` of the two blocks is a ``DecomposedRelationalDense`` (``layers/relational.py``), the subclass
that serves ``num_bases`` / ``num_blocks``; without these options it is the plain layer.
"""
import torch

from ... import _ffi
from ..base import GraphBaseLayer
from ..gather import GatherNodesOutgoing, GatherNodesSelection
from ..modules import Activation, Dense, LazyAdd, LazyMultiply, _activation_name
from ..pooling import PoolingLocalMessages
from ..relational import DecomposedRelationalDense

FUSED_RELATIONAL_SIZES = {"widths": (32, 64, 128), "max_relations": _ffi.MP_RELCONV_MAX_RELATIONS}   # csrc/mp_rgcn.hip


def fused_relational_supported(node_width, units, num_relations, message_activation="linear", activations=(),
                               edge_weight_width=1, dtype="float32"):
    """True when one block with these sizes runs on ``mp_relational_conv_f32`` (the configuration decides).
    ``activations``: every other activation of the block (output, self-loop Dense or modulation)."""
    s = FUSED_RELATIONAL_SIZES
    if node_width is None or units is None or int(node_width) not in s["widths"] or int(units) not in s["widths"]:
        return False
    if num_relations is None or not 1 <= int(num_relations) <= s["max_relations"]:
        return False
    if _activation_name(message_activation) not in ("linear", None):
        return False
    if edge_weight_width is None or int(edge_weight_width) != 1:
        return False
    if any(_activation_name(act) not in _ffi.ACTIVATION_CODES for act in activations):
        return False
    return dtype in ("float32", torch.float32)


def _detached(t):
    return None if t is None else t.detach().contiguous()


def relational_conv_values(mode, nodes, edge_index, relations, weights, kernel, bias, units, act, self_loop=None,
                           modulation=None):
    """One block on ``mp_relational_conv_f32``.  ``kernel`` (R, K, U) is the effective message kernel; ``self_loop`` =
    ``(W0, b0, act0)`` (RGCN), ``modulation`` = ``(Wg, bg, Wt, bt, act_m)`` (FiLM).  Returns the updated nodes."""
    what = "the fused relational step"
    plan = edge_index.index_plan(nodes)
    plan.validate()
    hv, rv = nodes.values, relations.values
    _ffi.require_device(hv, rv, kernel)
    n, e, k = plan.N, plan.M, int(hv.shape[-1])
    if hv.dtype != torch.float32 or hv.dim() != 2 or plan.K != 2 or n != int(hv.shape[0]):
        raise ValueError("%s expects float32 nodes (batch, [N], F) and an edge index of two columns" % what)
    if rv.dim() != 1 or int(rv.shape[0]) != e:
        raise ValueError("%s: %d relations for %d edges" % (what, int(rv.numel()), e))
    if tuple(kernel.shape[1:]) != (k, units):
        raise ValueError("%s: kernel %s for node width %d and %d units" % (what, tuple(kernel.shape), k, units))
    relc = rv.contiguous() if rv.dtype == torch.int64 else rv.to(torch.int64).contiguous()
    wv = None
    if weights is not None:
        wv = weights.values
        if wv.dtype != torch.float32 or wv.numel() != e:
            raise ValueError("%s expects float32 edge weights (batch, [M], 1)" % what)
        wv = _detached(wv)
    if n >= 2 ** 31 - 16 or e >= 2 ** 31 - 256:
        raise ValueError("%s indexes nodes and edges with 32 bits" % what)
    ptr0, perm0, _ = plan.csr(0)
    w0 = b0 = wg = bg = wt = bt = None
    act0 = act_m = "linear"
    if self_loop is not None:
        w0, b0, act0 = self_loop
    if modulation is not None:
        wg, bg, wt, bt, act_m = modulation
    out = torch.empty((n, units), dtype=torch.float32, device=hv.device)
    _ffi.call("mp_relational_conv_f32", mode, _ffi.ptr(_detached(hv)), n, k, _ffi.ptr(plan.cols), e, _ffi.ptr(ptr0),
              _ffi.ptr(perm0), _ffi.ptr(relc), _ffi.ptr(wv), int(kernel.shape[0]), _ffi.ptr(_detached(kernel)),
              _ffi.ptr(_detached(bias)), units, _ffi.ptr(_detached(w0)), _ffi.ptr(_detached(b0)),
              _ffi.activation_code(_activation_name(act0)), _ffi.ptr(_detached(wg)), _ffi.ptr(_detached(bg)),
              _ffi.ptr(_detached(wt)), _ffi.ptr(_detached(bt)), _ffi.activation_code(_activation_name(act_m)),
              _ffi.activation_code(_activation_name(act)), 0.05, _ffi.ptr(out), _ffi.stream())
    return nodes.with_values(out)


class _RelationalStep(GraphBaseLayer):
    """What both blocks share: the route switch and the tape check."""

    # Dense, RelationalDense, the gathers, the elementwise layers and the pooling carry their rules
    weight_gradients = True

    def _init_route(self):
        self.use_fused_relational = True
        self.fused_relational = None      # decided in build(): the sizes fit the fused kernel

    def needs_grad(self, *inputs):
        """The kernel reads the weights in place and has no reverse rule: any tape steps aside to the layer sequence."""
        from ...autograd import needs_grad
        return needs_grad(*inputs) or needs_grad(*[t for _, t in self.weights if t is not None])

    def _fused(self, kwargs, *inputs):
        return bool(self.fused_relational and self.use_fused_relational and not kwargs and not self.needs_grad(*inputs))


class RGCNStep(_RelationalStep):
    r"""One block of RGCN (kgcnn/literature/RGCN.py:96-103): ``step([nodes, edge_index, edge_weights, edge_relations])``
    returns ``act(sum_{e -> i} w_e (n_j W_{rel e} + b) + Dense(n_i))``.  Sublayers in the reference's creation order:
    ``Dense(**dense_kwargs)``, then ``RelationalDense(**dense_relation_kwargs)``.  ``use_fused_relational`` (default True):
    sizes that fit ``fused_relational_supported`` run on ``mp_relational_conv_f32`` outside a tape (``fused_relational``,
    decided in ``build``)."""

    def __init__(self, dense_kwargs=None, dense_relation_kwargs=None, activation_kwargs=None, **kwargs):
        super().__init__(**kwargs)
        self.dense_kwargs = dict(dense_kwargs) if dense_kwargs is not None else {"units": 64}
        self.dense_relation_kwargs = dict(dense_relation_kwargs) if dense_relation_kwargs is not None \
            else {"units": 64, "num_relations": 20}
        self.activation_kwargs = dict(activation_kwargs) if activation_kwargs is not None else {"activation": "swish"}
        self.lay_gather = GatherNodesOutgoing()
        self.lay_dense = Dense(**self.dense_kwargs)
        self.lay_relational = DecomposedRelationalDense(**self.dense_relation_kwargs)
        self.lay_mul = LazyMultiply()
        self.lay_pool = PoolingLocalMessages(pooling_method="sum")
        self.lay_add = LazyAdd()
        self.lay_act = Activation(**self.activation_kwargs)
        self._init_route()

    @property
    def units(self):
        return self.lay_relational.units

    def build(self, input_shape):
        """``input_shape``: ``[nodes (batch, None, K), edge_index, edge_weights (batch, None, 1), edge_relations]``; creates
        every weight (so ``set_weights`` works before a first call) and decides the route."""
        super().build(input_shape)
        width = int(input_shape[0][-1])
        self.lay_dense.ensure_built((None, None, width))
        self.lay_relational.ensure_built([(None, None, width), (None, None)])
        weight_width = input_shape[2][-1] if len(input_shape[2]) > 2 else None
        rel = self.lay_relational
        self.fused_relational = bool(
            self.lay_dense.units == rel.units and
            fused_relational_supported(width, rel.units, rel.num_relations, rel.activation,
                                       (self.lay_dense.activation, self.lay_act.activation), weight_width, self.dtype))

    def call(self, inputs, **kwargs):
        n, edi, edge_weights, edge_relations = inputs
        if self._fused(kwargs, n.values, edge_weights.values):
            rel, dense = self.lay_relational, self.lay_dense
            return relational_conv_values(_ffi.MP_RELCONV_RGCN, n, edi, edge_relations, edge_weights,
                                          rel.effective_kernel(), rel.bias, rel.units, self.lay_act.activation,
                                          self_loop=(dense.kernel, dense.bias, dense.activation))
        n_j = self.lay_gather([n, edi], **kwargs)
        h0 = self.lay_dense(n, **kwargs)
        h_j = self.lay_relational([n_j, edge_relations], **kwargs)
        m = self.lay_mul([h_j, edge_weights], **kwargs)
        h = self.lay_pool([n, m, edi], **kwargs)
        return self.lay_act(self.lay_add([h, h0], **kwargs), **kwargs)

    def get_config(self):
        config = super().get_config()
        config.update({"dense_kwargs": dict(self.dense_kwargs), "dense_relation_kwargs": dict(self.dense_relation_kwargs),
                       "activation_kwargs": dict(self.activation_kwargs)})
        return config


class GNNFilmStep(_RelationalStep):
    r"""One block of GNNFilm (kgcnn/literature/GNNFilm.py:93-102): ``step([nodes, edge_index, edge_relations])`` returns
    ``act(sum_{e -> i} [gamma_e * (n_j W_{rel e} + b) + beta_e])`` with ``gamma_e`` / ``beta_e`` two
    ``RelationalDense(**dense_modulation_kwargs)`` of the receiver's features.  Sublayers in the reference's creation order:
    gamma, beta, then the message ``RelationalDense(**dense_relation_kwargs)``.  ``use_fused_relational`` as ``RGCNStep``."""

    def __init__(self, dense_relation_kwargs=None, dense_modulation_kwargs=None, activation_kwargs=None, **kwargs):
        super().__init__(**kwargs)
        self.dense_relation_kwargs = dict(dense_relation_kwargs) if dense_relation_kwargs is not None \
            else {"units": 64, "num_relations": 20}
        self.dense_modulation_kwargs = dict(dense_modulation_kwargs) if dense_modulation_kwargs is not None \
            else {"units": 64, "num_relations": 20, "activation": "sigmoid"}
        self.activation_kwargs = dict(activation_kwargs) if activation_kwargs is not None else {"activation": "swish"}
        self.lay_gather = GatherNodesSelection(selection_index=[0, 1])
        self.lay_gamma = DecomposedRelationalDense(**self.dense_modulation_kwargs)
        self.lay_beta = DecomposedRelationalDense(**self.dense_modulation_kwargs)
        self.lay_relational = DecomposedRelationalDense(**self.dense_relation_kwargs)
        self.lay_mul = LazyMultiply()
        self.lay_add = LazyAdd()
        self.lay_pool = PoolingLocalMessages(pooling_method="sum")
        self.lay_act = Activation(**self.activation_kwargs)
        self._init_route()

    @property
    def units(self):
        return self.lay_relational.units

    def build(self, input_shape):
        """``input_shape``: ``[nodes (batch, None, K), edge_index, edge_relations]``; creates every weight and decides the
        route."""
        super().build(input_shape)
        width = int(input_shape[0][-1])
        for lay in (self.lay_gamma, self.lay_beta, self.lay_relational):
            lay.ensure_built([(None, None, width), (None, None)])
        rel, mod = self.lay_relational, self.lay_gamma
        self.fused_relational = bool(
            mod.units == rel.units and mod.num_relations == rel.num_relations and
            fused_relational_supported(width, rel.units, rel.num_relations, rel.activation,
                                       (mod.activation, self.lay_act.activation), 1, self.dtype))

    def call(self, inputs, **kwargs):
        n, edi, edge_relations = inputs
        if self._fused(kwargs, n.values):
            rel, gamma, beta = self.lay_relational, self.lay_gamma, self.lay_beta
            return relational_conv_values(_ffi.MP_RELCONV_FILM, n, edi, edge_relations, None, rel.effective_kernel(),
                                          rel.bias, rel.units, self.lay_act.activation,
                                          modulation=(gamma.effective_kernel(), gamma.bias, beta.effective_kernel(),
                                                      beta.bias, gamma.activation))
        n_i, n_j = self.lay_gather([n, edi], **kwargs)
        gamma = self.lay_gamma([n_i, edge_relations], **kwargs)
        beta = self.lay_beta([n_i, edge_relations], **kwargs)
        h_j = self.lay_relational([n_j, edge_relations], **kwargs)
        m = self.lay_mul([h_j, gamma], **kwargs)
        m = self.lay_add([m, beta], **kwargs)
        h = self.lay_pool([n, m, edi], **kwargs)
        return self.lay_act(h, **kwargs)

    def get_config(self):
        config = super().get_config()
        config.update({"dense_relation_kwargs": dict(self.dense_relation_kwargs),
                       "dense_modulation_kwargs": dict(self.dense_modulation_kwargs),
                       "activation_kwargs": dict(self.activation_kwargs)})
        return config
