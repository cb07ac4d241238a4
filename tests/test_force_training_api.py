"""Training on forces without a GPU: the second-derivative entry points of csrc/mp_backward2.hip are declared, bound and
validate their arguments; ``EnergyForceModel.compile`` / ``train_on_batch`` reject what they cannot do; the force-target
unpadding and the Keras gradient clipping.  No kernel is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from gcnn_keras_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mp_activation_grad2_f32", "mp_gauss_basis_grad2_f32", "mp_euclidean_norm_grad2_f32")


def test_new_symbols_in_header_and_ctypes_table():
    raw = _ffi.HEADER_TEXT
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _ffi.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _ffi.declared_symbols(), name
        assert hasattr(lib, name), name
    # the declarations cite the reference lines whose derivatives they reverse
    for cite in ("geom.py:567-571", "geom.py:181-193", "modules.py:15-90"):
        assert cite in raw, cite


def test_argument_errors_return_einval():
    lib = _ffi.lib()
    # unknown activation code, negative size
    assert lib.mp_activation_grad2_f32(99, 0.0, None, None, None, None, None, 4, None) == _ffi.MP_EINVAL
    assert b"mp_activation_grad2_f32" in lib.mp_last_error()
    assert lib.mp_activation_grad2_f32(-1, 0.0, None, None, None, None, None, 4, None) == _ffi.MP_EINVAL
    assert lib.mp_activation_grad2_f32(2, 0.0, None, None, None, None, None, -1, None) == _ffi.MP_EINVAL
    # an output asked for, inputs missing
    host = (ctypes.c_float * 4)()
    buf = ctypes.cast(host, ctypes.c_void_p)   # never written: the checks fail first
    assert lib.mp_activation_grad2_f32(2, 0.0, None, None, None, buf, None, 4, None) == _ffi.MP_EINVAL
    # gauss: no bins, zero sigma
    assert lib.mp_gauss_basis_grad2_f32(None, 4, 0, 5.0, 0.4, 0.0, None, None, None, None, None) == _ffi.MP_EINVAL
    assert lib.mp_gauss_basis_grad2_f32(None, 4, 25, 5.0, 0.0, 0.0, None, None, None, None, None) == _ffi.MP_EINVAL
    assert lib.mp_gauss_basis_grad2_f32(None, 4, 25, 5.0, 0.4, 0.0, None, None, buf, None, None) == \
        _ffi.MP_EINVAL
    # norm: invert and square_norm have no second derivative here, even for an empty call; bad sizes
    for flags in (1, 8, 1 | 2, 8 | 4, 16):
        assert lib.mp_euclidean_norm_grad2_f32(None, None, None, 0, 3, 1, flags, None, None, None) == _ffi.MP_EINVAL
    assert b"mp_euclidean_norm_grad2_f32" in lib.mp_last_error()
    assert lib.mp_euclidean_norm_grad2_f32(None, None, None, 4, 0, 1, 0, None, None, None) == _ffi.MP_EINVAL
    assert lib.mp_euclidean_norm_grad2_f32(None, None, None, -1, 3, 1, 0, None, None, None) == _ffi.MP_EINVAL
    with pytest.raises(ValueError):
        _ffi.check(lib.mp_euclidean_norm_grad2_f32(None, None, None, 4, 3, 1, 8, None, None, None))


def test_zero_sized_calls_need_no_device():
    lib = _ffi.lib()
    for act in range(10):
        assert lib.mp_activation_grad2_f32(act, 0.05, None, None, None, None, None, 0, None) == _ffi.MP_OK
    assert lib.mp_gauss_basis_grad2_f32(None, 0, 25, 5.0, 0.4, 0.0, None, None, None, None, None) == _ffi.MP_OK
    for flags in (0, 2, 4, 6):
        assert lib.mp_euclidean_norm_grad2_f32(None, None, None, 0, 3, 1, flags, None, None, None) == _ffi.MP_OK
    # no output asked for: nothing to do
    assert lib.mp_activation_grad2_f32(2, 0.0, None, None, None, None, None, 16, None) == _ffi.MP_OK


def _efm(**kw):
    from gcnn_keras_amd.literature import Schnet
    from gcnn_keras_amd.model.force import EnergyForceModel
    return EnergyForceModel(model_energy=Schnet.make_model(depth=1), coordinate_input=1, energy_output=0,
                            output_as_dict=False, output_squeeze_states=True, is_physical_force=False, **kw)


def test_compile_rejects_bad_losses_and_weights():
    model = _efm()
    with pytest.raises(ValueError):
        model.compile(loss=["mean_squared_error"] * 3)
    with pytest.raises(ValueError):
        model.compile(loss=["mean_squared_error"])
    with pytest.raises(ValueError):
        model.compile(loss=["mean_squared_error"] * 2, loss_weights=[1.0])
    with pytest.raises(ValueError):
        model.compile(loss=["mean_squared_error"] * 2, loss_weights=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError):
        model.compile(loss=["mean_squared_error", "force_of_doom"])
    with pytest.raises(ValueError):
        model.compile(loss="mean_squared_error", clipnorm=0.0)
    model.compile(optimizer="adam", loss=["mean_squared_error", "mean_squared_error"], loss_weights=[1 / 200, 199 / 200],
                  clipnorm=1.0)
    assert model.loss_weights == [1 / 200, 199 / 200] and model.clipnorm == 1.0
    assert isinstance(model.optimizer, torch.optim.Adam)
    assert [id(t) for t in model.optimizer.param_groups[0]["params"]] == \
        [id(t) for t in model.energy_model.trainable_weights]
    model.compile(optimizer="sgd", loss="mean_absolute_error")
    assert model.loss_weights == [1.0, 1.0] and model.clipnorm is None and len(model.loss) == 2


def test_trainable_weights_delegate_to_the_energy_model():
    model = _efm()
    assert [id(t) for t in model.trainable_weights] == [id(t) for t in model.energy_model.trainable_weights]
    model.requires_grad_(True)
    assert all(t.requires_grad for t in model.energy_model.trainable_weights)
    model.requires_grad_(False)
    assert not any(t.requires_grad for t in model.energy_model.trainable_weights)


def test_train_on_batch_before_compile_raises():
    with pytest.raises(RuntimeError):
        _efm().train_on_batch([None, None, None], [np.zeros((1, 1), np.float32), np.zeros((1, 3), np.float32)])


def test_unsupported_training_cases_raise():
    model = _efm(esp_input=3, esp_grad_input=4).compile(loss="mean_squared_error")
    with pytest.raises(NotImplementedError):
        model.train_on_batch([None] * 5, [np.zeros((1, 1), np.float32), np.zeros((1, 3), np.float32)])
    assert not any(t.requires_grad for t in model.trainable_weights)
    model = _efm().compile(loss="mean_squared_error")
    y = [np.zeros((1, 1), np.float32), np.zeros((1, 3), np.float32)]
    with pytest.raises(NotImplementedError):
        model.train_on_batch([None] * 3, y, sample_weight=[None, np.ones(1, np.float32)])
    with pytest.raises(NotImplementedError):
        model.train_on_batch([None] * 3, y, sample_weight=np.ones(1, np.float32))


def test_force_targets_ragged_flat_and_padded():
    from gcnn_keras_amd.model.losses import flat_target
    from gcnn_keras_amd.ragged import RaggedTensor
    splits = np.array([0, 2, 2, 5], np.int64)
    flat = np.arange(15, dtype=np.float32).reshape(5, 3)
    padded = np.full((3, 4, 3), 99.0, np.float32)
    for g in range(3):
        padded[g, :splits[g + 1] - splits[g]] = flat[splits[g]:splits[g + 1]]
    like = torch.zeros(5, 3)
    for target in (flat, torch.from_numpy(padded), padded, RaggedTensor(torch.from_numpy(flat), torch.from_numpy(splits))):
        got = flat_target(target, like, splits)
        assert torch.equal(got, torch.from_numpy(flat))
    # unsqueezed states axis: (N, 3, 1) output, (N, 3) or (B, Nmax, 3, 1) targets
    like3 = torch.zeros(5, 3, 1)
    assert torch.equal(flat_target(flat, like3, splits), torch.from_numpy(flat).view(5, 3, 1))
    assert torch.equal(flat_target(padded[..., None], like3, splits), torch.from_numpy(flat).view(5, 3, 1))
    with pytest.raises(ValueError):
        flat_target(padded[:, :1], like, splits)
    with pytest.raises(ValueError):
        flat_target(flat[:4], like, splits)


def test_clipnorm_is_keras_clip_by_norm():
    from gcnn_keras_amd.model.utils import clip_gradients
    a = torch.zeros(4, requires_grad=True)
    b = torch.zeros(2, 2, requires_grad=True)
    c = torch.zeros(3, requires_grad=True)
    a.grad = torch.tensor([3.0, 4.0, 0.0, 0.0])          # norm 5 -> scaled to 1
    b.grad = torch.tensor([[0.1, 0.2], [0.2, 0.0]])      # norm 0.3 -> untouched
    clip_gradients([a, b, c], 1.0)
    assert torch.allclose(a.grad, torch.tensor([0.6, 0.8, 0.0, 0.0]))
    assert torch.equal(b.grad, torch.tensor([[0.1, 0.2], [0.2, 0.0]]) * 1.0 / 1.0)
    assert c.grad is None
    before = a.grad.clone()
    clip_gradients([a], None)
    assert torch.equal(a.grad, before)


def test_model_compile_keeps_its_signature_and_takes_clipnorm():
    from gcnn_keras_amd.literature import Schnet
    model = Schnet.make_model(depth=1)
    assert model.compile(optimizer="adam", loss="mean_absolute_error").clipnorm is None
    assert model.compile(optimizer="sgd", loss="mean_absolute_error", clipnorm=2.0).clipnorm == 2.0
