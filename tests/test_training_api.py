"""Training interface without a GPU: the parameter-gradient entry points are declared, bound and validate their
arguments; ``Model.compile`` / ``train_on_batch`` reject what they cannot do; the weight-gradient guard of
``Layer.__call__`` fires before any device work.  No kernel is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from gcnn_keras_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mp_dense_wgrad_f32", "mp_dense_wgrad_ws_bytes", "mp_embedding_grad_f32", "mp_embedding_grad_ws_bytes",
               "mp_softmax_rows_grad_f32")


def _header_text():
    return _ffi.HEADER_TEXT


def test_new_symbols_in_header_and_ctypes_table():
    text = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    lib = _ffi.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _ffi.declared_symbols(), name
        assert hasattr(lib, name), name
    # the declarations cite the Keras tape they replace
    assert "kgcnn/layers/modules.py:15-90" in _header_text() and "train_qm.py:164-166" in _header_text()


def test_argument_errors_return_einval():
    lib = _ffi.lib()
    nbytes = ctypes.c_size_t(0)
    assert lib.mp_dense_wgrad_f32(None, 4, 0, None, 4, None, None, None, 0, None) == _ffi.MP_EINVAL
    assert b"mp_dense_wgrad_f32" in lib.mp_last_error()
    assert lib.mp_dense_wgrad_f32(None, -1, 4, None, 4, None, None, None, 0, None) == _ffi.MP_EINVAL
    assert lib.mp_dense_wgrad_f32(None, 4, 4, None, 0, None, None, None, 0, None) == _ffi.MP_EINVAL
    assert lib.mp_dense_wgrad_f32(None, 0, 4, None, 4, None, None, None, 0, None) == _ffi.MP_EINVAL   # no dW
    assert lib.mp_dense_wgrad_ws_bytes(10, 0, 4, ctypes.byref(nbytes)) == _ffi.MP_EINVAL
    assert lib.mp_dense_wgrad_ws_bytes(10, 4, 4, None) == _ffi.MP_EINVAL
    assert lib.mp_embedding_grad_f32(None, 4, None, 0, 8, None, 0, None, None) == _ffi.MP_EINVAL
    assert lib.mp_embedding_grad_f32(None, -1, None, 95, 8, None, 0, None, None) == _ffi.MP_EINVAL
    assert lib.mp_embedding_grad_ws_bytes(4, 0, ctypes.byref(nbytes)) == _ffi.MP_EINVAL
    assert lib.mp_softmax_rows_grad_f32(None, None, 4, 0, None, None) == _ffi.MP_EINVAL
    assert lib.mp_softmax_rows_grad_f32(None, None, 4, 7, None, None) == _ffi.MP_EINVAL
    with pytest.raises(ValueError):
        _ffi.check(lib.mp_softmax_rows_grad_f32(None, None, -1, 7, None, None))


def test_zero_sized_calls_need_no_device():
    lib = _ffi.lib()
    nbytes = ctypes.c_size_t(123)
    assert lib.mp_softmax_rows_grad_f32(None, None, 0, 7, None, None) == _ffi.MP_OK
    assert lib.mp_dense_wgrad_ws_bytes(0, 128, 128, ctypes.byref(nbytes)) == _ffi.MP_OK
    assert nbytes.value == 0
    assert lib.mp_embedding_grad_ws_bytes(0, 95, ctypes.byref(nbytes)) == _ffi.MP_OK


def test_wgrad_workspace_monotone_and_bounded():
    lib = _ffi.lib()

    def ws(r, k, u):
        n = ctypes.c_size_t(0)
        assert lib.mp_dense_wgrad_ws_bytes(r, k, u, ctypes.byref(n)) == _ffi.MP_OK
        return n.value

    for k, u in ((20, 128), (128, 128), (1433, 64), (3, 7), (1, 1), (64, 1)):
        prev = 0
        for r in list(range(0, 2000, 7)) + [26190, 10 ** 5, 2_500_000, 10 ** 7]:
            cur = ws(r, k, u)
            assert cur >= prev, (r, k, u)
            prev = cur
        # bounded: at most 512 slabs of dW + db, whatever R
        assert ws(10 ** 7, k, u) <= 512 * 4 * (k * u + u)
    assert ws(10 ** 7, 128, 128) == ws(10 ** 9, 128, 128)


def _schnet():
    from gcnn_keras_amd.literature import Schnet
    return Schnet.make_model(depth=1)


def test_compile_rejects_unknown_loss_and_optimizer():
    model = _schnet()
    with pytest.raises(ValueError):
        model.compile(optimizer="adam", loss="hinge_of_doom")
    with pytest.raises(ValueError):
        model.compile(optimizer="rmsprop_nope", loss="mean_absolute_error")
    with pytest.raises(ValueError):
        model.compile(optimizer=object(), loss="mean_absolute_error")
    model.compile(optimizer="adam", loss="mean_absolute_error")
    assert isinstance(model.optimizer, torch.optim.Adam)
    group = model.optimizer.param_groups[0]
    assert group["lr"] == 1e-3 and group["betas"] == (0.9, 0.999) and group["eps"] == 1e-7
    model.compile(optimizer="sgd", loss="categorical_crossentropy")
    assert isinstance(model.optimizer, torch.optim.SGD) and model.optimizer.param_groups[0]["lr"] == 0.01
    opt = torch.optim.SGD(model.trainable_weights, lr=0.5)
    assert model.compile(optimizer=opt, loss="mean_squared_error").optimizer is opt


def test_train_on_batch_before_compile_raises():
    model = _schnet()
    with pytest.raises(RuntimeError):
        model.train_on_batch([None, None, None], np.zeros((1, 1), np.float32))


def test_trainable_weights_and_requires_grad_switch():
    model = _schnet()
    ws = model.trainable_weights
    assert [id(t) for t in ws] == [id(t) for _, t in model.weights]
    assert not any(t.requires_grad for t in ws)
    model.requires_grad_(True)
    assert all(t.requires_grad for t in ws)
    # set_weights works on weights that require grad (runs under no_grad)
    model.set_weights([np.full(t.shape, 0.5, np.float32) for t in ws])
    assert all(float(t.detach().flatten()[0]) == 0.5 for t in ws if t.numel())
    model.requires_grad_(False)
    assert not any(t.requires_grad for t in ws)


def test_keras_losses():
    from gcnn_keras_amd.model.losses import get_loss
    p = torch.tensor([[0.2, 0.3, 0.5], [0.9, 0.05, 0.05]], dtype=torch.float64)
    y = torch.tensor([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0]], dtype=torch.float64)
    w = torch.tensor([1.0, 0.0], dtype=torch.float64)
    ce = get_loss("categorical_crossentropy")(p, y, w)
    assert abs(float(ce) - (-np.log(0.5) * 1.0 + 0.0) / 2) < 1e-12        # sum over batch size: weight 0 rows count
    mae = get_loss("mean_absolute_error")(p, y)
    assert abs(float(mae) - float((p - y).abs().mean())) < 1e-12
    mse = get_loss("mean_squared_error")(p, y, w)
    assert abs(float(mse) - float(((p - y) ** 2).mean(-1)[0]) / 2) < 1e-12
    with pytest.raises(ValueError):
        get_loss("nope")


def test_layer_without_weight_gradients_raises_in_grad_mode():
    from gcnn_keras_amd.layers.geom import BesselBasisLayer
    from gcnn_keras_amd.layers.modules import Dense
    lay = BesselBasisLayer(num_radial=4, cutoff=5.0)
    lay.ensure_built((None, None, 1))
    d = torch.ones(3, 1)
    lay.frequencies.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="BesselBasisLayer"):
        lay(d)
    with torch.no_grad():                  # no gradient asked: the layer runs (and, without a GPU, stops at the engine)
        with pytest.raises(_ffi.EngineError):
            lay(d)
    lay.frequencies.requires_grad_(False)
    with pytest.raises(_ffi.EngineError):   # frozen weights: no guard
        lay(d)
    dense = Dense(4)
    dense.ensure_built((None, 3))
    dense.kernel.requires_grad_(True)
    with pytest.raises(_ffi.EngineError):   # Dense has weight gradients: reaches the engine
        dense(torch.ones(2, 3))
