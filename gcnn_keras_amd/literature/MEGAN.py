"""MEGAN, the multi-explanation graph attention network (mirror of kgcnn/literature/MEGAN.py:23-483; Teufel et al. 2022)
on the engine's layers.

``MEGAN(units=[...], importance_channels=K, ...)`` stacks ``MultiHeadGATV2Layer`` blocks with ``K`` heads, sums their
attention logits into edge importances, forms node importances from them and from a Dense chain on the node embeddings,
pools the embeddings once per channel weighted by the node importances, and ends in an MLP.  The output is ``out``
``(batch, final_units[-1])`` or ``(out, node_importances (batch, [N], K), edge_importances (batch, [M], K))``.

Two route switches.  ``use_fused_attention`` covers the attention layers as in GAT (csrc/mp_gat.hip; they step aside on a
tape).  ``use_fused_readout`` covers the tail behind the last attention layer (csrc/mp_megan.hip): the importance Dense
launches plus two launches whatever ``K`` and the number of layers are, and two more in reverse - unlike the attention
block the readout carries its reverse rule (``autograd.MeganReadout``), so it also serves training.  Every other
configuration takes the layer sequence, one engine call per Keras layer.

The reference as it executes, kept here: ``use_final_activation`` of the attention layers stays at its default ``True``;
``final_biases`` is computed but every final Dense gets ``use_bias``; the result of the final dropout is discarded;
``importance_dropout_rate`` is stored and unused; the embedding exists only for a truthy ``input_embedding``;
``regression_reference`` is added only with ``regression_limits``.  ``Dropout`` is the inference identity; the sparsity
regulariser enters the loss in ``train_on_batch`` rather than in every forward.
"""
import numpy as np
import torch

from .. import _ffi
from ..layers.base import GraphBaseLayer
from ..layers.conv.gat_conv import MultiHeadGATV2Layer
from ..layers.modules import (Activation, Dense, Dropout, LazyAverage, LazyConcatenate, OptionalInputEmbedding,
                              _activation_name, binary_values, concat_last, split_last)
from ..layers.pooling import PoolingLocalEdges, PoolingNodes
from ..model.utils import RouteSwitchModel, clip_gradients
from ..ops.activ import apply_activation
from ..ops.segment import reduce_op_code

__model_version__ = "2022.12.15"


def shifted_sigmoid(x, shift=5, multiplier=1):
    """``sigmoid((x - shift) / multiplier)`` (kgcnn/literature/MEGAN.py:23-24).  Device tensors go through the engine's
    elementwise kernels (with their reverse rules); host tensors and arrays - the label side - are evaluated on the host."""
    if torch.is_tensor(x) and x.is_cuda:
        v = x if x.dim() else x.reshape(1)
        const = lambda c: torch.full((1,) * v.dim(), float(c), dtype=torch.float32, device=v.device)
        v = binary_values(_ffi.MP_SUB, v, const(shift))
        if float(multiplier) != 1.0:
            v = binary_values(_ffi.MP_MUL, v, const(1.0 / float(multiplier)))
        return apply_activation("sigmoid", v).reshape(x.shape)
    if torch.is_tensor(x):
        return torch.sigmoid((x - shift) / multiplier)
    return 1.0 / (1.0 + np.exp(-(np.asarray(x) - shift) / multiplier))


class ExplanationSparsityRegularization(GraphBaseLayer):
    """``factor * mean |importances|`` (kgcnn/literature/MEGAN.py:27-40).  Keras' ``add_loss``: the value of the last call
    is kept in ``losses`` (one entry), and returned."""

    weight_gradients = True   # layers/base.py: the layer has no weights

    def __init__(self, factor: float = 1.0, **kwargs):
        super().__init__(**kwargs)
        self.factor = factor
        self.losses = []

    def call(self, inputs, **kwargs):
        from ..model.losses import mean_absolute_error
        values = inputs if torch.is_tensor(inputs) else inputs.values
        # the loss is the project's loss plumbing on a model output (model/losses.py): mean |ni - 0|
        loss = mean_absolute_error(values, torch.zeros_like(values)) * self.factor
        self.losses = [loss]
        return loss

    def get_config(self):
        config = super().get_config()
        config.update({"factor": self.factor})
        return config


class MEGAN(RouteSwitchModel):
    """MEGAN: Multi Explanation Graph Attention Network (constructor arguments and defaults of the reference,
    kgcnn/literature/MEGAN.py:55-126).  Inputs ``[node_attributes, edge_attributes, edge_indices]``.

    ``model.use_fused_attention`` / ``model.use_fused_readout`` switch the routes (a flip drops the captured graphs, and
    both are part of a captured graph's identity); ``model.fused_readout`` tells whether the configuration fits the fused
    readout.  Built for given widths by ``make_model`` / ``build(node_width, edge_width)``; otherwise on the first call
    (``compile`` needs the weights, so call or build the model first)."""

    __kgcnn_model_version__ = __model_version__
    switch_attr, switch_layers_attr = "use_fused_attention", "attention_layers"

    def __init__(self,
                 # convolutional network related arguments
                 units,
                 activation: str = "kgcnn>leaky_relu",
                 use_bias: bool = True,
                 dropout_rate: float = 0.0,
                 use_edge_features: bool = True,
                 input_embedding: dict = None,
                 # node/edge importance related arguments
                 importance_units=(),
                 importance_channels: int = 2,
                 importance_activation: str = "sigmoid",
                 importance_dropout_rate: float = 0.0,
                 importance_factor: float = 0.0,
                 importance_multiplier: float = 10.0,
                 sparsity_factor: float = 0.0,
                 concat_heads: bool = True,
                 # mlp tail end related arguments
                 final_units=(1,),
                 final_dropout_rate: float = 0.0,
                 final_activation: str = "linear",
                 final_pooling: str = "sum",
                 regression_limits=None,
                 regression_reference=None,
                 return_importances: bool = True,
                 name: str = "MEGAN",
                 **kwargs):
        if kwargs:
            raise TypeError("Unknown MEGAN arguments %s" % sorted(kwargs))
        self.units = list(units)
        self.activation = activation
        self.use_bias = use_bias
        self.dropout_rate = dropout_rate
        self.use_edge_features = use_edge_features
        self.input_embedding = input_embedding
        self.importance_units = list(importance_units)
        self.importance_channels = int(importance_channels)
        self.importance_activation = importance_activation
        self.importance_dropout_rate = importance_dropout_rate
        self.importance_factor = importance_factor
        self.importance_multiplier = importance_multiplier
        self.sparsity_factor = sparsity_factor
        self.concat_heads = concat_heads
        self.final_units = list(final_units)
        self.final_dropout_rate = final_dropout_rate
        self.final_activation = final_activation
        self.final_pooling = final_pooling
        self.regression_limits = regression_limits
        self.regression_reference = regression_reference
        self.return_importances = return_importances
        if len(self.units) == 0 or len(self.final_units) == 0:
            raise ValueError("MEGAN needs at least one attention layer and one final layer")
        if self.regression_limits is not None and self.importance_factor != 0 and self.importance_channels != 2:
            # regression_augmentation has two columns (below / above the reference): one explanation channel each
            raise ValueError("MEGAN: the explanation step of a regression takes importance_channels=2, got %d"
                             % self.importance_channels)

        # ~ MAIN CONVOLUTIONAL / ATTENTION LAYERS
        layers = []
        if self.input_embedding:
            self.embedding_nodes = OptionalInputEmbedding(**self.input_embedding["node"])
            layers.append(self.embedding_nodes)
        self.attention_layers = [
            MultiHeadGATV2Layer(units=u, num_heads=self.importance_channels, use_edge_features=self.use_edge_features,
                                activation=self.activation, use_bias=self.use_bias, has_self_loops=True,
                                concat_heads=self.concat_heads)
            for u in self.units]
        self.lay_dropout = Dropout(rate=self.dropout_rate)

        # ~ EDGE IMPORTANCES
        self.lay_act_importance = Activation(activation=self.importance_activation)
        self.lay_concat_alphas = LazyConcatenate(axis=-1)
        self.lay_pool_edges_in = PoolingLocalEdges(pooling_method="mean", pooling_index=0)
        self.lay_pool_edges_out = PoolingLocalEdges(pooling_method="mean", pooling_index=1)
        self.lay_average = LazyAverage()

        # ~ NODE IMPORTANCES
        self.node_importance_units = self.importance_units + [self.importance_channels]
        self.node_importance_acts = ["relu" for _ in self.importance_units] + ["linear"]
        self.node_importance_layers = [Dense(units=u, activation=act, use_bias=use_bias)
                                       for u, act in zip(self.node_importance_units, self.node_importance_acts)]
        self.lay_sparsity = ExplanationSparsityRegularization(factor=self.sparsity_factor)

        # ~ OUTPUT / MLP TAIL END
        self.lay_pool_out = PoolingNodes(pooling_method=self.final_pooling)
        self.lay_concat_out = LazyConcatenate(axis=-1)
        self.lay_final_dropout = Dropout(rate=self.final_dropout_rate)
        self.final_acts = ["relu" for _ in self.final_units]
        self.final_acts[-1] = self.final_activation
        self.final_biases = [True for _ in self.final_units]
        self.final_biases[-1] = False       # computed and never used, as in the reference
        self.final_layers = [Dense(units=u, activation=act, use_bias=use_bias)
                             for u, act in zip(self.final_units, self.final_acts)]

        if self.regression_limits is not None:
            self.regression_width = np.abs(self.regression_limits[1] - self.regression_limits[0])

        layers += self.attention_layers + self.node_importance_layers + self.final_layers
        super().__init__(name, self._forward_all, layers, config=self.get_config(), auto_graph=True)
        self._use_fused_readout = True
        self.last_readout_route = None    # "fused" | "layers": the route of the last forward's tail
        self.last_exp_loss = None

    # -- configuration -----------------------------------------------------------------------------------------------------
    def get_config(self):
        return {
            "units": self.units,
            "activation": self.activation,
            "use_bias": self.use_bias,
            "dropout_rate": self.dropout_rate,
            "use_edge_features": self.use_edge_features,
            "importance_units": self.importance_units,
            "importance_channels": self.importance_channels,
            "importance_activation": self.importance_activation,
            "importance_dropout_rate": self.importance_dropout_rate,
            "importance_factor": self.importance_factor,
            "importance_multiplier": self.importance_multiplier,
            "sparsity_factor": self.sparsity_factor,
            "concat_heads": self.concat_heads,
            "final_units": self.final_units,
            "final_dropout_rate": self.final_dropout_rate,
            "final_activation": self.final_activation,
            "final_pooling": self.final_pooling,
            "regression_limits": self.regression_limits,
            "regression_reference": self.regression_reference,
            "return_importances": self.return_importances,
            "input_embedding": self.input_embedding,
        }

    @property
    def doing_regression(self) -> bool:
        return self.regression_limits is not None

    def build(self, node_width, edge_width):
        """Create every weight for node features of ``node_width`` (behind the embedding, if any) and edge features of
        ``edge_width``."""
        if self.input_embedding:
            self.embedding_nodes.ensure_built((None, None))
        width = int(node_width)
        for lay in self.attention_layers:
            lay.ensure_built([(None, None, width), (None, None, int(edge_width)), (None, None, 2)])
            width = lay.units * lay.num_heads if self.concat_heads else lay.units
        self.embedding_width = width
        imp = width
        for lay in self.node_importance_layers:
            lay.ensure_built((None, None, imp))
            imp = lay.units
        out = width * self.importance_channels
        for lay in self.final_layers:
            lay.ensure_built((None, out))
            out = lay.units
        return self

    # -- routes ------------------------------------------------------------------------------------------------------------
    def _switches(self):
        return tuple(bool(lay.use_fused_attention) for lay in self.attention_layers) + (bool(self._use_fused_readout),)

    def _set_attention(self, value):
        if any(bool(lay.use_fused_attention) != bool(value) for lay in self.attention_layers):
            self.release_graphs()
        for lay in self.attention_layers:
            lay.use_fused_attention = bool(value)

    use_fused_attention = property(lambda self: all(lay.use_fused_attention for lay in self.attention_layers),
                                   _set_attention)

    def _set_readout(self, value):
        if bool(value) != bool(self._use_fused_readout):
            self.release_graphs()
        self._use_fused_readout = bool(value)

    use_fused_readout = property(lambda self: bool(self._use_fused_readout), _set_readout)

    def fused_readout_supported(self, width=None, dtype=torch.float32):
        """The configuration (and, when given, the embedding width ``W`` and dtype) fits csrc/mp_megan.hip."""
        from ..autograd import MEGAN_READOUT_SIZES as s
        pools = (self.lay_pool_edges_in, self.lay_pool_edges_out)
        return (dtype in ("float32", torch.float32)
                and 1 <= self.importance_channels <= s["max_channels"]
                and 1 <= len(self.units) <= s["max_layers"]
                and (width is None or (int(width) >= 4 and int(width) % 4 == 0 and int(width) <= s["max_width"]))
                and self.final_pooling in ("sum", "mean")
                and _activation_name(self.importance_activation) == "sigmoid"
                and [p.pooling_index for p in pools] == [0, 1]
                and all(p.pooling_method == "mean" and p.has_unconnected and not p.is_sorted for p in pools))

    @property
    def fused_readout(self):
        """Decided by the build: the tail runs on the fused readout when the switch is on."""
        last = self.attention_layers[-1]
        width = last.units * last.num_heads if self.concat_heads else last.units
        return bool(self.fused_readout_supported(width))

    def _readout_route(self, x, alphas):
        xv = x.values
        return (self._use_fused_readout and xv.dim() == 2 and self.fused_readout_supported(int(xv.shape[1]), xv.dtype)
                and all(a.values.dtype == torch.float32 for a in alphas))

    # -- forward -----------------------------------------------------------------------------------------------------------
    def _importance_chain(self, x, last_linear):
        """The node-importance Dense chain on the embeddings; ``last_linear`` stops before the importance activation."""
        t = x
        for lay in self.node_importance_layers:
            t = lay(t)
        return t if last_linear else self.lay_act_importance(t)

    def _tail_layers(self, node_input, x, alphas, edi):
        """kgcnn/literature/MEGAN.py:274-308, one engine call per Keras layer."""
        k = self.importance_channels
        # the (M, K, 1) logits of the layers concatenated on the last axis and summed over it: a left fold over (M, K)
        total = alphas[0].values.reshape(alphas[0].values.shape[0], k)
        for a in alphas[1:]:
            total = binary_values(_ffi.MP_ADD, total, a.values.reshape(a.values.shape[0], k))
        edge_importances = self.lay_act_importance(edi.with_values(total))
        pooled_in = self.lay_pool_edges_in([node_input, edge_importances, edi])
        pooled_out = self.lay_pool_edges_out([node_input, edge_importances, edi])
        pooled = self.lay_average([pooled_out, pooled_in])
        tilde = self._importance_chain(x, last_linear=False)
        node_importances = x.with_values(binary_values(_ffi.MP_MUL, tilde.values, pooled.values))
        outs = []
        slices = split_last(node_importances.values, k) if k > 1 else [node_importances.values]
        for col in slices:                                # (N, 1): tf.expand_dims(node_importances[:, :, k], -1)
            outs.append(self.lay_pool_out(x.with_values(binary_values(_ffi.MP_MUL, x.values, col))))
        rows = min(int(o.shape[0]) for o in outs)
        out = concat_last([o[:rows] for o in outs]) if k > 1 else outs[0]
        return out, node_importances, edge_importances

    def _tail_fused(self, x, alphas, edi):
        """The same on csrc/mp_megan.hip: the importance Dense launches plus two."""
        from ..autograd import MeganReadout, megan_readout_values, needs_grad
        z = self._importance_chain(x, last_linear=True).values
        xv = x.values
        _ffi.require_device(xv, edi.values)
        plan = edi.index_plan(x)
        plan.validate()
        g = x.nrows()
        op = reduce_op_code(self.final_pooling)
        logits = [a.values for a in alphas]
        if needs_grad(xv, z, *logits):
            out, ni, ei = MeganReadout.apply(xv, z, plan, x.row_splits, g, op, *logits)
        else:
            out, ni, ei, _ = megan_readout_values(xv.detach().contiguous(), z.detach().contiguous(), plan, x.row_splits, g,
                                                  op, [t.detach().contiguous() for t in logits])
        splits = x.row_splits_host()
        rows = g
        while rows > 0 and splits[rows] == splits[rows - 1]:     # trailing empty graphs, as layers/pooling.py drops them
            rows -= 1
        if rows != g:
            out = out[:rows]
        return out, x.with_values(ni), edi.with_values(ei)

    def _forward_all(self, inputs, **kwargs):
        """``(out, node_importances, edge_importances)`` of one batch."""
        node_input, edge_input, edi = inputs
        if self.input_embedding:
            node_input = self.embedding_nodes(node_input)
        alphas = []
        x = node_input
        for lay in self.attention_layers:
            x, alpha = lay([x, edge_input, edi])
            alphas.append(alpha)
        if self._readout_route(x, alphas):
            self.last_readout_route = "fused"
            out, node_importances, edge_importances = self._tail_fused(x, alphas, edi)
        else:
            self.last_readout_route = "layers"
            out, node_importances, edge_importances = self._tail_layers(node_input, x, alphas, edi)
        for lay in self.final_layers:
            out = lay(out)       # the reference's final dropout discards its result
        if self.doing_regression:
            ref = torch.full((1, 1), float(self.regression_reference), dtype=torch.float32, device=out.device)
            out = binary_values(_ffi.MP_ADD, out, ref)
        return out, node_importances, edge_importances

    def _check_dropout(self, what):
        if self.dropout_rate or self.final_dropout_rate:
            raise NotImplementedError("MEGAN: %s with dropout_rate=%r, final_dropout_rate=%r needs training-mode dropout, "
                                      "which the engine does not have (inference treats dropout as the identity)"
                                      % (what, self.dropout_rate, self.final_dropout_rate))

    def __call__(self, inputs, training=False, return_importances=False):
        if training:
            self._check_dropout("a call with training=True")
        out, node_importances, edge_importances = super().__call__(inputs)
        if self.last_route == "graph":
            # the replayed graph writes into its own buffers: hand out copies of the two ragged outputs as well
            node_importances = node_importances.with_values(node_importances.values.clone())
            edge_importances = edge_importances.with_values(edge_importances.values.clone())
        if self.return_importances or return_importances:
            return out, node_importances, edge_importances
        return out

    def explain_importances(self, x, **kwargs):
        _, node_importances, edge_importances = self(x, return_importances=True)
        return node_importances, edge_importances

    # -- training ----------------------------------------------------------------------------------------------------------
    def regression_augmentation(self, out_true):
        """For true values ``(B, 1)``: ``samples (B, 2)``, the distance to ``regression_reference`` in units of half the
        regression width times ``importance_multiplier`` (twice), and ``mask (B, 2)`` = [below, above the reference]
        (kgcnn/literature/MEGAN.py:329-357).  Label side: torch ops where ``out_true`` lives."""
        t = out_true if torch.is_tensor(out_true) else torch.as_tensor(np.asarray(out_true, dtype=np.float32))
        t = t.to(torch.float32).reshape(-1, 1)
        ref = float(self.regression_reference)
        dist = (t - ref).abs() * float(self.importance_multiplier) / (0.5 * float(self.regression_width))
        lo = torch.where(t < ref, 1.0, 0.0).to(torch.float32)
        hi = torch.where(t > ref, 1.0, 0.0).to(torch.float32)
        return torch.cat([dist, dist], dim=-1), torch.cat([lo, hi], dim=-1)

    def explanation_loss(self, node_importances, y):
        """The explanation-only term of the train step (kgcnn/literature/MEGAN.py:397-429), before ``importance_factor``:
        ``outs[b, k]`` = ``final_pooling`` of channel ``k`` of the node importances over graph ``b`` (one graph pool for
        all channels); regression ``K * MAE(samples * mask, outs * mask)``, classification ``BCE(y, sigmoid(outs -
        importance_multiplier))``.  Pool, mask product, shift and sigmoid are engine kernels with their reverse rules."""
        from ..model.losses import _values, binary_crossentropy, mean_absolute_error
        outs = self.lay_pool_out(node_importances)
        if self.doing_regression:
            samples, mask = self.regression_augmentation(_values(y, outs))
            samples, mask = samples.to(outs.device)[:outs.shape[0]], mask.to(outs.device)[:outs.shape[0]]
            masked = binary_values(_ffi.MP_MUL, outs, mask.contiguous())
            return self.importance_channels * mean_absolute_error(masked, samples * mask)
        pred = shifted_sigmoid(outs, shift=self.importance_multiplier, multiplier=1)
        return binary_crossentropy(pred, y)

    def total_loss(self, x, y, sample_weight=None):
        """``(loss, exp_loss)`` on the tape: compiled loss + ``sparsity_factor * mean |ni|`` + ``importance_factor *``
        the explanation loss; ``exp_loss`` is the last term (``None`` when ``importance_factor == 0``)."""
        out, node_importances, _ = self._forward_all(x)
        loss = self._loss_fn(out, y, sample_weight)
        loss = loss + self.lay_sparsity(node_importances)
        exp_loss = None
        if self.importance_factor != 0:
            exp_loss = self.explanation_loss(node_importances, y) * self.importance_factor
            loss = loss + exp_loss
        return loss, exp_loss

    def train_on_batch(self, x, y, sample_weight=None):
        """The reference's ``train_step`` (kgcnn/literature/MEGAN.py:359-451): one optimizer step on the total loss.
        Returns the total loss before the step, and with ``importance_factor != 0`` the list ``[loss, exp_loss]``
        (``exp_loss`` includes ``importance_factor``, as the reference's metric does); ``last_exp_loss`` keeps it."""
        if self.optimizer is None:
            raise RuntimeError("Model %s: call compile(optimizer, loss) before train_on_batch" % self.name)
        if self.return_importances:
            raise NotImplementedError("MEGAN: training with return_importances=True (supervised explanations, a "
                                      "three-part target) is not implemented; build the model with "
                                      "return_importances=False to train it")
        self._check_dropout("train_on_batch")
        weights = self.trainable_weights
        saved = [t.requires_grad for t in weights]
        try:
            for t in weights:
                t.requires_grad_(True)
            self.optimizer.zero_grad(set_to_none=True)
            with torch.enable_grad():
                loss, exp_loss = self.total_loss(x, y, sample_weight)
                loss.backward()
            clip_gradients(weights, getattr(self, "clipnorm", None))
            self.optimizer.step()
        finally:
            for t, flag in zip(weights, saved):
                t.requires_grad_(flag)
        self.lay_sparsity.losses = []
        if exp_loss is None:
            self.last_exp_loss = None
            return float(loss.detach())
        self.last_exp_loss = float(exp_loss.detach())
        return [float(loss.detach()), self.last_exp_loss]

    def fit(self, x, y, batch_size=32, epochs=1, shuffle=True, validation_data=None, sample_weight=None, callbacks=None,
            initial_epoch=0, verbose=0, seed=None):
        """``Model.fit``; the ``History`` holds ``exp_loss`` next to ``loss`` when ``importance_factor != 0``."""
        from ..model.loop import fit
        if self.optimizer is None:
            raise RuntimeError("Model %s: call compile(optimizer, loss) before fit" % self.name)
        names = ["loss", "exp_loss"] if self.importance_factor != 0 else ["loss"]
        return fit(self, names, x, y, batch_size=batch_size, epochs=epochs, shuffle=shuffle,
                   validation_data=validation_data, sample_weight=sample_weight, callbacks=callbacks,
                   initial_epoch=initial_epoch, verbose=verbose, seed=seed)

    def evaluate(self, x, y, batch_size=32, sample_weight=None):
        """The compiled loss of ``out`` over the data set (the importances are not part of it)."""
        from ..model.loop import evaluate
        if self._loss_fn is None:
            raise RuntimeError("Model %s: call compile(optimizer, loss) before evaluate" % self.name)
        with torch.no_grad():
            return evaluate(lambda xb, yb, swb: self._loss_fn(RouteSwitchModel.__call__(self, xb)[0], yb, swb), x, y,
                            batch_size, sample_weight)


def _feature_width(spec, embedding):
    if len(spec["shape"]) < 2:
        if not embedding:
            raise ValueError("MEGAN: a (None,) input needs an input_embedding")
        return embedding["output_dim"]
    return spec["shape"][-1]


def make_model(inputs=None, **kwargs):
    r"""``MEGAN(**kwargs)`` built for the widths in ``inputs`` (kgcnn/literature/MEGAN.py:461-483): a list of three input
    dictionaries, ``[node_attributes (None, F) or (None,), edge_attributes (None, Fe), edge_indices (None, 2)]``."""
    megan = MEGAN(**kwargs)
    if inputs is not None:
        embedding = (megan.input_embedding or {}).get("node")
        node_width = _feature_width(inputs[0], embedding)
        edge_width = inputs[1]["shape"][-1] if len(inputs[1]["shape"]) >= 2 else 1
        megan.build(node_width, edge_width)
    megan.__kgcnn_model_version__ = __model_version__
    return megan
