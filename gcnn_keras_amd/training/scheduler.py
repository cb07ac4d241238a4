"""Learning-rate schedulers of kgcnn/training/scheduler.py as callbacks of ``Model.fit`` / ``EnergyForceModel.fit``.

``LinearLearningRateScheduler`` states the rule of kgcnn/training/scheduler.py:245-300 (written independently of it): the
rate is ``learning_rate_start`` for ``epoch < epo_min``, then falls linearly and reaches ``learning_rate_stop`` at epoch
``epo``; it is never below ``eps``.  Keras' ``LearningRateScheduler`` sets the optimizer's rate at the beginning of an
epoch and logs it as ``lr`` at its end; here the optimizer is the ``torch.optim.Optimizer`` of ``model.compile``, and
every parameter group receives the rate."""
from ..model.loop import Callback


class LinearLearningRateScheduler(Callback):

    def __init__(self, learning_rate_start: float = 1e-3, learning_rate_stop: float = 1e-5, epo_min: int = 0,
                 epo: int = 500, verbose: int = 0, eps: float = 1e-8):
        self.learning_rate_start = learning_rate_start
        self.learning_rate_stop = learning_rate_stop
        self.epo = epo
        self.epo_min = epo_min
        self.verbose = verbose
        self.eps = float(eps)

    def schedule_epoch_lr(self, epoch, lr=None):
        """Rate of ``epoch`` (counted from 0); ``lr``, the current rate, is not used."""
        if epoch < self.epo_min:
            out = float(self.learning_rate_start)
        else:
            slope = (self.learning_rate_start - self.learning_rate_stop) / (self.epo - self.epo_min)
            out = float(self.learning_rate_start - slope * (epoch - self.epo_min))
        return max(out, self.eps)

    def _optimizer(self):
        optimizer = getattr(self.model, "optimizer", None)
        if optimizer is None or not hasattr(optimizer, "param_groups"):
            raise ValueError("LinearLearningRateScheduler needs a compiled model (a torch optimizer with param_groups)")
        return optimizer

    def on_epoch_begin(self, epoch, logs=None):
        groups = self._optimizer().param_groups
        rate = self.schedule_epoch_lr(epoch, groups[0]["lr"] if groups else None)
        for group in groups:
            group["lr"] = rate
        if self.verbose > 0:
            print("Epoch %05d: LinearLearningRateScheduler setting learning rate to %s." % (epoch + 1, rate))

    def on_epoch_end(self, epoch, logs=None):
        if logs is not None:
            groups = self._optimizer().param_groups
            logs["lr"] = float(groups[0]["lr"]) if groups else None

    def get_config(self):
        return {"verbose": self.verbose, "learning_rate_start": self.learning_rate_start,
                "learning_rate_stop": self.learning_rate_stop, "epo": self.epo, "epo_min": self.epo_min, "eps": self.eps}
