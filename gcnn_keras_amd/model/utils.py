"""Model keyword handling with the contract of kgcnn/model/utils.py:69-142 (written independently of it):

* ``update_model_kwargs_logic(defaults, user, update_recursive)`` returns a fresh dictionary = deep copy of the defaults
  overlaid with the user's entries; a top-level user key that the defaults do not know raises ``ValueError``; where both
  sides hold a dictionary the overlay recurses (``update_recursive`` levels deep, below that it replaces wholesale); a
  dictionary replaced by a non-dictionary, and a nested key the defaults lack, are accepted with a warning.
* ``@update_model_kwargs(model_default)`` applies that to the keyword arguments of a ``make_model`` and, like the
  reference, takes the logger level from the merged ``verbose`` entry; positional arguments pass through untouched
  (with an error log, since they cannot be merged).
"""
import copy
import functools
import logging
from math import inf

module_logger = logging.getLogger(__name__)
module_logger.setLevel(logging.WARNING)


def _overlay(base, patch, levels_left):
    """Write ``patch`` over ``base`` in place; ``levels_left`` counts how many more dictionary levels may be merged
    rather than replaced."""
    for name, new_value in patch.items():
        old_value = base.get(name, _overlay)        # the function object doubles as the 'absent' marker
        if old_value is _overlay:
            module_logger.warning("Model kwargs: Unknown key %s with value %s", name, new_value)
            base[name] = new_value
        elif isinstance(old_value, dict) and isinstance(new_value, dict) and levels_left > 0:
            _overlay(old_value, new_value, levels_left - 1)
        else:
            if isinstance(old_value, dict) and not isinstance(new_value, dict):
                module_logger.warning("Model kwargs: Overwriting dictionary of %s with %s", name, new_value)
            base[name] = new_value
    return base


def update_model_kwargs_logic(default_kwargs: dict = None, user_kwargs: dict = None, update_recursive=inf):
    defaults = default_kwargs or {}
    user = user_kwargs or {}
    unknown = [name for name in user if name not in defaults]
    if unknown:
        raise ValueError("Model kwarg %s not in default arguments %s" % (unknown[0], list(defaults)))
    return _overlay(copy.deepcopy(defaults), user, update_recursive)


def update_model_kwargs(model_default, update_recursive=inf):
    def decorate(make_model):
        @functools.wraps(make_model)
        def with_defaults(*args, **kwargs):
            merged = update_model_kwargs_logic(model_default, kwargs, update_recursive)
            if "verbose" in merged:
                module_logger.setLevel(merged["verbose"])
            module_logger.info("Updated model kwargs: %s", merged)
            if args:
                module_logger.error("Can only update kwargs, not %s", args)
            return make_model(*args, **merged)
        return with_defaults
    return decorate


def make_optimizer(optimizer, weights):
    """``"adam"`` / ``"sgd"`` with Keras' defaults (Adam lr 1e-3, betas (0.9, 0.999), epsilon 1e-7; SGD lr 0.01) over
    ``weights``, or a ``torch.optim.Optimizer`` as given."""
    import torch
    if isinstance(optimizer, str):
        name = optimizer.lower()
        if name == "adam":
            return torch.optim.Adam(weights, lr=1e-3, betas=(0.9, 0.999), eps=1e-7)
        if name == "sgd":
            return torch.optim.SGD(weights, lr=0.01)
        raise ValueError("Unknown optimizer %r (use 'adam', 'sgd' or a torch.optim.Optimizer)" % (optimizer,))
    if not isinstance(optimizer, torch.optim.Optimizer):
        raise ValueError("optimizer must be 'adam', 'sgd' or a torch.optim.Optimizer, got %r" % (optimizer,))
    return optimizer


def check_clipnorm(clipnorm):
    if clipnorm is None:
        return None
    clipnorm = float(clipnorm)
    if not clipnorm > 0.0:
        raise ValueError("clipnorm must be positive, got %r" % (clipnorm,))
    return clipnorm


def clip_gradients(weights, clipnorm):
    """Keras OptimizerV2 ``clipnorm`` (``tf.clip_by_norm`` per gradient tensor): g * c / max(|g|_2, c).  Optimizer
    plumbing on the gradients, in place; nothing happens for ``clipnorm=None``."""
    if clipnorm is None:
        return
    import torch
    for t in weights:
        g = t.grad
        if g is None:
            continue
        norm = g.square().sum().sqrt()
        g.copy_(g * clipnorm / torch.clamp(norm, min=clipnorm))


class Model:
    """Minimal stand-in for ``ks.models.Model``: an ordered list of layers plus a forward function.

    ``auto_graph``: a layer-path model issues one engine call per Keras layer (a dozen to a few hundred launches), and at
    QM9 / Cora sizes the host cannot keep the GPU busy that way.  With ``auto_graph=True`` the model remembers, per
    distinct input set (identified by the storage of its tensors), how often it was called: the first call runs eagerly
    (building and caching the index plans on the ragged inputs), the second captures the same call sequence into ONE HIP
    graph (``engine.GraphedModel``), later calls replay it and return a fresh copy of the output.  Calls that ask for
    gradients (inputs or weights that require grad, in grad mode), pass keyword arguments, or whose capture fails (a
    layer that needs a host read per call) stay eager.

    Training (the Keras ``compile`` / ``fit`` pair, kgcnn/training/train_qm.py:159-166): ``compile(optimizer, loss)`` then
    ``train_on_batch(x, y, sample_weight)`` - one step of zero grads, layer-path forward, loss, backward (the engine's
    reverse rules, weight gradients included) and ``optimizer.step()``.  The weights require grad only inside the step, so
    between steps every call takes the same (fused / graph-replayed) route as an untrained model.
    """

    def __init__(self, name, forward, layers, config=None, auto_graph=False, max_graphs=4):
        self.name = name
        self._forward = forward
        self.layers = layers
        self.config = config or {}
        self.auto_graph = bool(auto_graph)
        self.max_graphs = int(max_graphs)
        self._graphs = {}      # input identity -> [calls, GraphedModel | None | False]
        self.last_route = None  # "eager" | "graph"
        self.optimizer = None
        self.loss = None
        self._loss_fn = None
        self.clipnorm = None

    def __call__(self, inputs, **kwargs):
        if self.auto_graph and not kwargs and not self._weights_need_grad():
            key = self._graph_key(inputs)
            if key is not None:
                return self._call_graphed(key, inputs)
        self.last_route = "eager"
        return self._forward(inputs, **kwargs)

    # -- graph replay of re-bound inputs ----------------------------------------------------------------------------------
    @staticmethod
    def _graph_key(inputs):
        import torch
        from .. import _ffi
        from ..ragged import RaggedTensor
        if not _ffi.has_gpu() or not isinstance(inputs, (list, tuple)):
            return None
        key = []
        for x in inputs:
            parts = (x.values, x.row_splits) if isinstance(x, RaggedTensor) else (x,)
            for t in parts:
                if not torch.is_tensor(t) or not t.is_cuda or (torch.is_grad_enabled() and t.requires_grad):
                    return None
                key.append((t.data_ptr(), tuple(t.shape), t._version if t.dtype == torch.int64 else 0))
        return tuple(key)

    def _call_graphed(self, key, inputs):
        from ..ragged import RaggedTensor
        entry = self._graphs.get(key)
        if entry is None:
            while len(self._graphs) >= self.max_graphs:
                self._graphs.pop(next(iter(self._graphs)))
            entry = self._graphs[key] = [0, None, inputs]   # the entry keeps the inputs alive: addresses stay an identity
        entry[0] += 1
        if entry[0] == 1 or entry[1] is False:
            self.last_route = "eager"
            return self._forward(inputs)
        if entry[1] is None:
            from ..engine import GraphedModel
            try:
                entry[1] = GraphedModel(self._forward, inputs, grad=False, layers=self.layers)
            except Exception:   # e.g. a layer that reads a size back per call cannot be captured: stay eager
                import torch
                torch.cuda.synchronize()
                entry[1] = False
                self.last_route = "eager"
                return self._forward(inputs)
        out = entry[1]()
        self.last_route = "graph"
        if isinstance(out, RaggedTensor):
            return out.with_values(out.values.clone())
        if isinstance(out, (list, tuple)):
            return type(out)(o.clone() if hasattr(o, "clone") else o for o in out)
        return out.clone()

    def release_graphs(self):
        self._graphs.clear()

    def _weights_need_grad(self):
        import torch
        if not torch.is_grad_enabled():
            return False
        for lay in self.layers:
            for _, t in lay.weights:
                if t is not None and t.requires_grad:
                    return True
        return False

    # -- the Keras loop over a resident data set (model/loop.py) ------------------------------------------------------------
    def predict(self, x, batch_size=None, **kwargs):
        """``batch_size=None``: one call on ``x``, ``kwargs`` passed through.  With an integer: ``x`` is the whole data
        set (device tensors, ``MemoryGraphList.tensor(...)``), served in order ``batch_size`` graphs per model call on the
        current stream; the results are assembled on the device into what one call over the data set returns."""
        if batch_size is None:
            return self(x, **kwargs)
        from .loop import predict
        return predict(self, x, batch_size, kwargs)

    def evaluate(self, x, y, batch_size=32, sample_weight=None):
        """The compiled loss over the data set: mean over the batches, weighted by graphs per batch (Keras)."""
        import torch
        from .loop import evaluate
        if self._loss_fn is None:
            raise RuntimeError("Model %s: call compile(optimizer, loss) before evaluate" % self.name)
        with torch.no_grad():
            return evaluate(lambda xb, yb, swb: self._loss_fn(self(xb), yb, swb), x, y, batch_size, sample_weight)

    def fit(self, x, y, batch_size=32, epochs=1, shuffle=True, validation_data=None, sample_weight=None, callbacks=None,
            initial_epoch=0, verbose=0, seed=None):
        """Keras ``fit`` over a resident data set: per epoch the batches of ``data.batching.batch_ids(G, batch_size,
        shuffle, seed, epoch)``, each cut out on the GPU and given to ``train_on_batch``; returns a ``History``
        (``loss``, ``val_loss`` with ``validation_data=(x, y[, sample_weight])``, ``lr`` when a callback logs it)."""
        from .loop import fit
        if self.optimizer is None:
            raise RuntimeError("Model %s: call compile(optimizer, loss) before fit" % self.name)
        return fit(self, ["loss"], x, y, batch_size=batch_size, epochs=epochs, shuffle=shuffle,
                   validation_data=validation_data, sample_weight=sample_weight, callbacks=callbacks,
                   initial_epoch=initial_epoch, verbose=verbose, seed=seed)

    @property
    def weights(self):
        out = []
        for lay in self.layers:
            out.extend((lay.name + "/" + n, t) for n, t in lay.weights)
        return out

    @property
    def trainable_weights(self):
        """The weight tensors in ``weights`` order (the Keras name)."""
        return [t for _, t in self.weights]

    def requires_grad_(self, flag=True):
        """Switch ``requires_grad`` of every weight (for a hand-written torch training loop).  While on, calls in grad
        mode take the layer path, which records the weights on the tape."""
        for t in self.trainable_weights:
            t.requires_grad_(bool(flag))
        return self

    def get_weights(self):
        return [t.detach().cpu().numpy() for _, t in self.weights]

    # -- training --------------------------------------------------------------------------------------------------------
    def compile(self, optimizer="adam", loss="mean_absolute_error", clipnorm=None):
        """``optimizer``: a ``torch.optim.Optimizer`` over ``trainable_weights``, or ``"adam"`` / ``"sgd"`` with Keras'
        defaults (Adam lr 1e-3, betas (0.9, 0.999), epsilon 1e-7; SGD lr 0.01).  ``loss``: ``"mean_absolute_error"``,
        ``"mean_squared_error"``, ``"categorical_crossentropy"`` or ``"binary_crossentropy"`` (Keras semantics, reduction sum over batch size).
        ``clipnorm``: clip every gradient tensor to this L2 norm before the step (Keras OptimizerV2 ``clipnorm``)."""
        from .losses import get_loss
        loss_fn = get_loss(loss)
        self.optimizer = make_optimizer(optimizer, self.trainable_weights)
        self.loss, self._loss_fn, self.clipnorm = loss, loss_fn, check_clipnorm(clipnorm)
        return self

    def train_on_batch(self, x, y, sample_weight=None):
        """One optimizer step on ``(x, y)``; returns the loss before the step (a Python float)."""
        import torch
        if self.optimizer is None:
            raise RuntimeError("Model %s: call compile(optimizer, loss) before train_on_batch" % self.name)
        weights = self.trainable_weights
        saved = [t.requires_grad for t in weights]
        try:
            for t in weights:
                t.requires_grad_(True)
            self.optimizer.zero_grad(set_to_none=True)
            with torch.enable_grad():
                pred = self._forward(x)
                loss = self._loss_fn(pred, y, sample_weight)
                loss.backward()
            clip_gradients(weights, getattr(self, "clipnorm", None))
            self.optimizer.step()
        finally:
            for t, flag in zip(weights, saved):
                t.requires_grad_(flag)
        return float(loss.detach())

    def set_weights(self, arrays):
        ws = self.weights
        if len(ws) != len(arrays):
            raise ValueError("Model %s expects %d weight arrays, got %d" % (self.name, len(ws), len(arrays)))
        import numpy as np
        import torch
        for (n, t), a in zip(ws, arrays):
            a = np.asarray(a, dtype=np.float32)
            if tuple(a.shape) != tuple(t.shape):
                raise ValueError("Shape mismatch for %s: %s vs %s" % (n, tuple(a.shape), tuple(t.shape)))
            with torch.no_grad():
                t.copy_(torch.from_numpy(a))


class RouteSwitchModel(Model):
    """``Model`` over layers that each carry a boolean route switch, e.g. ``use_fused_gate``: the model-level switch sets
    it on every one of them and drops the captured HIP graphs, which hold the route they were captured on.  A subclass
    names the layers' attribute (``switch_attr``) and the model attribute that lists the layers (``switch_layers_attr``)
    and exposes ``RouteSwitchModel.switch`` under the switch's name."""

    switch_attr = None
    switch_layers_attr = None

    def _switches(self):
        return tuple(getattr(lay, self.switch_attr) for lay in getattr(self, self.switch_layers_attr))

    def _set_switch(self, value):
        if any(flag != bool(value) for flag in self._switches()):
            self.release_graphs()
        for lay in getattr(self, self.switch_layers_attr):
            setattr(lay, self.switch_attr, bool(value))

    switch = property(lambda self: all(self._switches()), _set_switch)

    def _graph_key(self, inputs):
        # the route is part of the identity of a captured graph (a per-layer switch flipped behind the model's back)
        key = Model._graph_key(inputs)
        return None if key is None else key + (self._switches(),)
