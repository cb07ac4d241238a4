"""``EnergyForceModel`` (mirror of kgcnn/model/force.py:11-242): wraps an energy model and returns forces as the
negative derivative of the energy w.r.t. the input coordinates.

The reference pads the coordinates, records a ``GradientTape`` and calls ``batch_jacobian`` (force.py:152-186).  Graphs
of a batch are independent, so that jacobian is one reverse pass per energy state with an all-ones upstream gradient;
here ``torch.autograd`` is the tape and every forward / backward computation is an engine kernel
(``gcnn_keras_amd.autograd``).  The fork's QM/MM inputs are honoured: with ``esp_input`` / ``esp_grad_input`` named, the
force gains the chain term ``dE/desp * desp/dr`` (force.py:153-158, 179-186).  Energy models that bring a fused reverse
pass (PaiNN: ``gcnn_keras_amd/fused_painn.py``) skip the tape altogether: energy and forces come from one HIP graph.

Training (the fork's force_schnet.py:163-205, 262): ``compile(optimizer, loss=[energy, force], loss_weights)`` then
``train_on_batch(x, [energy, force])``.  The force enters the loss, so the reverse pass is recorded itself
(``create_graph=True``) and differentiated once more: the second-order rules of ``gcnn_keras_amd.autograd``.
"""
import importlib

import torch

from ..layers.casting import ChangeTensorType


def get_model_class(module_name: str, class_name: str):
    """``kgcnn.model.utils.get_model_class`` (kgcnn/model/utils.py:17-39) for this package's ``literature`` modules."""
    if module_name.startswith("kgcnn."):
        module_name = "gcnn_keras_amd." + module_name[len("kgcnn."):]
    elif "." not in module_name:
        module_name = "gcnn_keras_amd.literature." + module_name
    return getattr(importlib.import_module(module_name), class_name or "make_model")


class EnergyForceModel:

    def __init__(self, model_energy=None, coordinate_input=1, esp_input=None, esp_grad_input=None, energy_output=1,
                 output_as_dict: bool = True, ragged_validate: bool = False, output_to_tensor: bool = True,
                 output_squeeze_states: bool = False, nested_model_config: bool = True,
                 is_physical_force: bool = True, **kwargs):
        if model_energy is None:
            raise ValueError("Require valid model in `model_energy` for force prediction.")
        self._model_energy = model_energy
        if isinstance(model_energy, dict):
            cls = get_model_class(model_energy["module_name"], model_energy.get("class_name", "make_model"))
            self.energy_model = cls(**model_energy["config"])
        elif callable(model_energy):
            self.energy_model = model_energy
        else:
            raise TypeError("Input `model_energy` must be dict or a model.")
        if output_as_dict is True and energy_output != 0:
            # same quirk as the reference (force.py:115-117)
            print("Kgcnn warning: energy-model returns more than just energy, setting output_as_dict as False")
            output_as_dict = False
        self.ragged_validate = ragged_validate
        self.coordinate_input = coordinate_input
        self.esp_input = esp_input
        self.esp_grad_input = esp_grad_input
        self.energy_output = energy_output
        self.output_as_dict = output_as_dict
        self.output_to_tensor = output_to_tensor
        self.output_squeeze_states = output_squeeze_states
        self.is_physical_force = is_physical_force
        self.nested_model_config = nested_model_config
        self.fused = None   # False: always take the tape + layer-by-layer reverse pass
        self.cast_coordinates = ChangeTensorType(input_tensor_type="ragged", output_tensor_type="tensor")

    def __call__(self, inputs, **kwargs):
        """inputs: list for the energy model; the ragged coordinates ``(batch, [N], 3)`` sit at ``coordinate_input``.
        Returns ``{"energy", "force"}`` or ``(outputs, force)`` like the reference (force.py:195-201)."""
        x = inputs[self.coordinate_input]
        fused = self._fused_energy_force(inputs, kwargs)
        if fused is not None:
            return fused
        outputs, eng, de_dr = self._tape(inputs, kwargs)
        force = x.with_values(de_dr.contiguous())
        if self.output_to_tensor:
            force = self.cast_coordinates(force)
        eng = eng.detach()
        if self.output_as_dict:
            return {"energy": eng, "force": force}
        if isinstance(outputs, list):
            return [o.detach() if torch.is_tensor(o) else o for o in outputs] + [force]
        return eng, force

    # -- the Keras loop over a resident data set (model/loop.py) ------------------------------------------------------------
    def predict(self, x, batch_size=None, **kwargs):
        """``batch_size=None``: one call on ``x``.  With an integer the data set ``x`` is served in order, ``batch_size``
        graphs per call; energies land in one ``(G, states)`` tensor, ragged forces keep the coordinates' splits, padded
        forces ``(B, Nmax_b, 3)`` land in one zero-filled ``(G, Nmax, 3)``."""
        if batch_size is None:
            return self(x, **kwargs)
        from .loop import predict
        return predict(self, x, batch_size, kwargs)

    def _batch_losses(self, x, y, sample_weight):
        """``[total, energy_loss, force_loss]`` of one batch as device scalars: the force pass without ``create_graph``."""
        from .losses import flat_target
        sw_energy = self._energy_sample_weight(sample_weight)
        _, eng, de_dr = self._tape(x, {})
        f_true = flat_target(y[1], de_dr, x[self.coordinate_input].row_splits_host())
        loss_e = self._loss_fns[0](eng.detach(), y[0], sw_energy)
        loss_f = self._loss_fns[1](de_dr.detach(), f_true, None)
        return [loss_e * self.loss_weights[0] + loss_f * self.loss_weights[1], loss_e, loss_f]

    def evaluate(self, x, y, batch_size=32, sample_weight=None):
        """``[total, energy_loss, force_loss]`` of the compiled losses over the data set (mean over the batches, weighted
        by graphs per batch).  ``y = [energy (G, states), force RaggedTensor (G, [N], 3)]``."""
        from .loop import evaluate
        self._check_training_call("evaluate", y)
        return evaluate(self._batch_losses, x, y, batch_size, sample_weight)

    def fit(self, x, y, batch_size=32, epochs=1, shuffle=True, validation_data=None, sample_weight=None, callbacks=None,
            initial_epoch=0, verbose=0, seed=None):
        """Keras ``fit`` of the two-output model over a resident data set (see ``Model.fit``); the ``History`` holds
        ``loss``, ``energy_loss`` and ``force_loss`` (the fork names its outputs ``energy`` and ``force``) and their
        ``val_`` twins."""
        from .loop import fit
        self._check_training_call("fit", y)
        return fit(self, ["loss", "energy_loss", "force_loss"], x, y, batch_size=batch_size, epochs=epochs,
                   shuffle=shuffle, validation_data=validation_data, sample_weight=sample_weight, callbacks=callbacks,
                   initial_epoch=initial_epoch, verbose=verbose, seed=seed)

    def _check_training_call(self, what, y):
        if getattr(self, "optimizer", None) is None:
            raise RuntimeError("EnergyForceModel: call compile(optimizer, loss) before %s" % what)
        if self.esp_input is not None and self.esp_grad_input is not None:
            raise NotImplementedError("training through the QM/MM esp branch is not implemented")
        if not isinstance(y, (list, tuple)) or len(y) != 2:
            raise ValueError("y must be [energy, force]")

    @staticmethod
    def _energy_sample_weight(sample_weight):
        if sample_weight is None:
            return None
        if not isinstance(sample_weight, (list, tuple)) or len(sample_weight) != 2 or sample_weight[1] is not None:
            raise NotImplementedError("sample_weight on the force output is not implemented; pass [w_energy, None]")
        return sample_weight[0]

    def _tape(self, inputs, kwargs, create_graph=False):
        """Energy model on the tape, then ``de_dr`` = the flat force values ``(N, 3[, states])`` with the wrapper's sign
        and state-axis conventions.  ``create_graph``: the reverse pass is recorded too (a loss on the force)."""
        from ..autograd import input_grads_only
        x = inputs[self.coordinate_input]
        inputs_energy = list(inputs)
        x_req = x.values.detach().clone().requires_grad_(True)
        inputs_energy[self.coordinate_input] = x.with_values(x_req)
        # QM/MM branch of the fork (force.py:153-158, 165-168): the electrostatic potential of the MM charges at the QM
        # atoms, esp (batch, [N]), is an input of the energy model that itself depends on the coordinates through its
        # precomputed gradient desp_dr (batch, [N], 3); both must be named for the branch to be taken, as in the reference.
        with_esp = self.esp_input is not None and self.esp_grad_input is not None
        watched = [x_req]
        if with_esp:
            esp, desp_dr = inputs[self.esp_input], inputs[self.esp_grad_input]
            esp_req = esp.values.detach().clone().requires_grad_(True)
            inputs_energy[self.esp_input] = esp.with_values(esp_req)
            watched.append(esp_req)
        with torch.enable_grad():
            outputs = self.energy_model(inputs_energy, **kwargs)
            eng = outputs[self.energy_output] if isinstance(outputs, list) else outputs
            if eng.dim() == 1:
                eng = eng.unsqueeze(-1)
            states = int(eng.shape[1])
            grads, grads_esp = [], []
            with input_grads_only():   # dE/dx only: the rules skip the weight gradients torch would throw away
                for s in range(states):
                    g = torch.autograd.grad(eng[:, s], watched, grad_outputs=torch.ones_like(eng[:, s]),
                                            retain_graph=create_graph or s + 1 < states, create_graph=create_graph,
                                            allow_unused=True)
                    grads.append(g[0] if g[0] is not None else torch.zeros_like(x_req))
                    if with_esp:
                        grads_esp.append(g[1] if g[1] is not None else torch.zeros_like(esp_req))
            de_dr = torch.stack(grads, dim=-1)  # (N, 3, states)
        if with_esp:
            # dE/dr += dE/desp * desp/dr (force.py:179-186): (N, 1, states) x (N, 3, 1) on the engine's broadcast kernel
            from .. import _ffi
            from ..layers.modules import _binary_raw
            n = int(x_req.shape[0])
            de_desp = torch.stack(grads_esp, dim=-1).reshape(n, 1, states).contiguous()
            chain = _binary_raw(_ffi.MP_MUL, de_desp, desp_dr.values.reshape(n, 3, 1).contiguous())
            de_dr = _binary_raw(_ffi.MP_ADD, de_dr.contiguous(), chain)
        if self.is_physical_force:
            de_dr = -de_dr
        if self.output_squeeze_states:
            de_dr = de_dr.squeeze(-1)
        return outputs, eng, de_dr

    # -- training --------------------------------------------------------------------------------------------------------
    @property
    def trainable_weights(self):
        """The energy model's weight tensors (``Model.trainable_weights``)."""
        return self.energy_model.trainable_weights

    def requires_grad_(self, flag=True):
        self.energy_model.requires_grad_(flag)
        return self

    def compile(self, optimizer="adam", loss="mean_absolute_error", loss_weights=None, clipnorm=None):
        """Keras ``compile`` of the two-output model (energy, force), in the order the wrapper returns them.

        ``loss``: one name or callable for both outputs, or a list / tuple of two (``"mean_absolute_error"``,
        ``"mean_squared_error"``, ...; see ``model.losses``).  ``loss_weights``: two floats, default ``[1, 1]``; the total
        loss is ``sum_i w_i loss_i`` (Keras).  ``optimizer``: ``"adam"`` / ``"sgd"`` with Keras' defaults or a
        ``torch.optim.Optimizer`` over ``trainable_weights``.  ``clipnorm``: every gradient tensor is clipped to this L2
        norm before the step (Keras OptimizerV2; the fork uses 1.0)."""
        from .losses import get_loss
        from .utils import check_clipnorm, make_optimizer
        losses = list(loss) if isinstance(loss, (list, tuple)) else [loss, loss]
        if len(losses) != 2:
            raise ValueError("EnergyForceModel has two outputs (energy, force): expected 2 losses, got %d" % len(losses))
        loss_fns = [get_loss(name) for name in losses]
        weights = [1.0, 1.0] if loss_weights is None else loss_weights
        if not isinstance(weights, (list, tuple)) or len(weights) != 2:
            raise ValueError("loss_weights must hold one weight per output (energy, force), got %r" % (loss_weights,))
        self.optimizer = make_optimizer(optimizer, self.trainable_weights)
        self.loss, self.loss_weights = losses, [float(w) for w in weights]
        self._loss_fns, self.clipnorm = loss_fns, check_clipnorm(clipnorm)
        return self

    def train_on_batch(self, x, y, sample_weight=None):
        """One optimizer step on ``x`` and ``y = [energy, force]``; returns ``[total, energy_loss, force_loss]`` (floats,
        before the step), as Keras does for a two-output model.

        The step: the energy model's layer path with every weight requiring grad, ``F = +-dE/dx`` recorded on the tape
        (``create_graph=True``; sign, ``energy_output`` and ``output_squeeze_states`` as in ``__call__``), the weighted
        loss, its gradient through the forward AND the reverse pass (second-order rules of ``gcnn_keras_amd.autograd``),
        optional clipping, ``optimizer.step()``; ``requires_grad`` of the weights is restored afterwards.

        Energy target: ``(batch, states)`` or ``(batch,)``.  Force target: a ``RaggedTensor`` with the coordinates' row
        splits, its flat ``(N, 3)`` values, or a padded ``(batch, Nmax, 3)`` array (unpadded with the coordinates' row
        splits).  The force loss is Keras' ragged reduction: the mean over the 3 components of an atom, then the mean over
        the N real atoms of the batch; padding never counts.  ``sample_weight``: ``None``, or ``[w_energy, None]`` with one
        weight per graph for the energy loss; weights on the force output (also a single array, which Keras would apply
        to both outputs) raise ``NotImplementedError``.  The QM/MM ``esp_input`` / ``esp_grad_input`` branch raises
        ``NotImplementedError`` as well."""
        from .losses import flat_target
        self._check_training_call("train_on_batch", y)
        sw_energy = self._energy_sample_weight(sample_weight)
        weights = self.trainable_weights
        saved = [t.requires_grad for t in weights]
        try:
            for t in weights:
                t.requires_grad_(True)
            self.optimizer.zero_grad(set_to_none=True)
            with torch.enable_grad():
                _, eng, de_dr = self._tape(x, {}, create_graph=True)
                coords = x[self.coordinate_input]
                f_true = flat_target(y[1], de_dr, coords.row_splits_host())
                loss_e = self._loss_fns[0](eng, y[0], sw_energy)
                loss_f = self._loss_fns[1](de_dr, f_true, None)
                total = loss_e * self.loss_weights[0] + loss_f * self.loss_weights[1]
                from ..autograd import coordinate_hessian_discarded
                with coordinate_hessian_discarded():   # only the weights' gradients are kept (HDNNP2nd's ACSF rules)
                    total.backward(inputs=[t for t in weights])
            from .utils import clip_gradients
            clip_gradients(weights, self.clipnorm)
            self.optimizer.step()
        finally:
            for t, flag in zip(weights, saved):
                t.requires_grad_(flag)
        return [float(total.detach()), float(loss_e.detach()), float(loss_f.detach())]

    def _fused_energy_force(self, inputs, kwargs=None):
        """Energy models that bring a fused reverse pass (``model.fused.energy_force``: PAiNN, gcnn_keras_amd/fused_painn.py)
        return energy and -dE/dx from one captured HIP graph instead of the tape + layer-by-layer reverse pass below.
        Taken when the wrapper is in its plain form: coordinates at input 1, one energy state, the energy model returning
        the energy alone, and no call argument that the energy model itself would have to see (``fused=False`` forces the
        layer path there, ``training=True`` belongs to the layer path: both take the tape here as well)."""
        route = getattr(self.energy_model, "fused", None)
        if kwargs and any(not (k == "training" and not v) for k, v in kwargs.items()):
            return None
        if (route is None or not hasattr(route, "energy_force") or self.fused is False or self.coordinate_input != 1
                or self.esp_input is not None or len(inputs) != 3 or not getattr(route, "single_state", False)
                or not route.accepts(list(inputs), with_forces=True)):
            return None
        eng, force = route.energy_force(list(inputs))
        x = inputs[self.coordinate_input]
        de_dr = force if self.is_physical_force else -force          # the kernels return the physical sign
        if not self.output_squeeze_states:
            de_dr = de_dr.unsqueeze(-1)
        force = x.with_values(de_dr.contiguous())
        if self.output_to_tensor:
            force = self.cast_coordinates(force)
        if self.output_as_dict:
            return {"energy": eng, "force": force}
        return eng, force

    def get_config(self):
        return {"model_energy": self._model_energy, "coordinate_input": self.coordinate_input,
                "esp_input": self.esp_input, "esp_grad_input": self.esp_grad_input,
                "output_as_dict": self.output_as_dict, "ragged_validate": self.ragged_validate,
                "output_to_tensor": self.output_to_tensor, "output_squeeze_states": self.output_squeeze_states,
                "nested_model_config": self.nested_model_config}
