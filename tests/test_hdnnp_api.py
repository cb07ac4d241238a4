"""HDNNP2nd without a GPU: the symmetry-function and relational entry points are declared, bound and validate their
arguments; the parameter tables and mapping tables are the reference's construction; the layers' config keys; what is
not implemented raises; the builder's assertions.  No kernel is launched."""
import ctypes
import os
import re

import numpy as np
import pytest

from gcnn_keras_amd import _ffi, synth
from gcnn_keras_amd.layers.conv.acsf_conv import ACSFConstNormalization, ACSFG2, ACSFG4
from gcnn_keras_amd.layers.mlp import RelationalMLP
from gcnn_keras_amd.layers.relational import RelationalDense
from gcnn_keras_amd.literature import HDNNP2nd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mp_acsf_g2_f32", "mp_acsf_g4_f32", "mp_acsf_g2_jvp_f32", "mp_acsf_g4_jvp_f32", "mp_acsf_g2_grad_f32",
               "mp_acsf_g4_grad_f32", "mp_acsf_grad_ws_bytes", "mp_relational_dense_f32",
               "mp_relational_dense_wgrad_ws_bytes", "mp_relational_dense_wgrad_f32")


def test_new_symbols_in_header_and_ctypes_table():
    raw = _ffi.HEADER_TEXT
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _ffi.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _ffi.declared_symbols(), name
        assert hasattr(lib, name), name
    for cite in ("acsf_conv.py:158-210", "acsf_conv.py:419-494", "relational.py:219-238"):
        assert cite in raw, cite


def test_argument_errors_return_einval():
    lib = _ffi.lib()
    host = (ctypes.c_float * 4)()
    buf = ctypes.cast(host, ctypes.c_void_p)
    # bad sizes, R*m beyond the LDS row, missing pointers
    assert lib.mp_acsf_g2_f32(None, None, 4, None, 0, None, None, None, None, 0, 5, 0, None, None) == _ffi.MP_EINVAL
    assert b"mp_acsf_g2_f32" in lib.mp_last_error()
    assert lib.mp_acsf_g2_f32(None, None, 4, None, 0, None, None, None, None, 100, 100, 0, None, None) == _ffi.MP_EINVAL
    assert lib.mp_acsf_g2_f32(buf, None, 4, None, 0, None, None, None, None, 4, 35, 0, buf, None) == _ffi.MP_EINVAL
    assert lib.mp_acsf_g4_f32(None, None, -1, None, 0, None, None, None, None, None, 10, 50, 0, 2.0, None, None) == \
        _ffi.MP_EINVAL
    assert lib.mp_acsf_g4_jvp_f32(buf, buf, 4, buf, 0, buf, None, buf, None, buf, 10, 50, 0, 2.0, None, None,
                                  None) == _ffi.MP_EINVAL
    assert lib.mp_acsf_grad_ws_bytes(10, 4, ctypes.byref(ctypes.c_size_t())) == _ffi.MP_EINVAL
    assert lib.mp_acsf_g4_grad_f32(buf, buf, 4, buf, 8, buf, None, buf, None, None, None, buf, buf, buf, 10, 50, 0,
                                   2.0, buf, None, 0, buf, None) == _ffi.MP_EINVAL
    # relational: unknown mode / activation, bias in the transposed mode, bad sizes
    assert lib.mp_relational_dense_f32(None, 4, 8, None, 30, None, None, 3, 0, 0.0, 2, None, None, None, None) == \
        _ffi.MP_EINVAL
    assert lib.mp_relational_dense_f32(None, 4, 8, None, 30, None, None, 3, 99, 0.0, 0, None, None, None, None) == \
        _ffi.MP_EINVAL
    assert lib.mp_relational_dense_f32(None, 4, 8, None, 30, None, buf, 3, 0, 0.0, 1, None, None, None, None) == \
        _ffi.MP_EINVAL
    assert lib.mp_relational_dense_f32(None, 4, 0, None, 30, None, None, 3, 0, 0.0, 0, None, None, None, None) == \
        _ffi.MP_EINVAL
    assert lib.mp_relational_dense_wgrad_f32(None, 4, 8, None, 0, None, 3, buf, None, None, 0, None) == _ffi.MP_EINVAL
    assert lib.mp_relational_dense_wgrad_f32(None, 4, 8, None, 30, None, 3, None, None, None, 0, None) == \
        _ffi.MP_EINVAL
    with pytest.raises(ValueError):
        _ffi.check(lib.mp_relational_dense_wgrad_f32(None, 4, 8, None, 30, None, 3, buf, None, None, 0, None))


def test_zero_sized_calls_need_no_device():
    lib = _ffi.lib()
    assert lib.mp_acsf_g2_f32(None, None, 0, None, 0, None, None, None, None, 4, 35, 0, None, None) == _ffi.MP_OK
    assert lib.mp_acsf_g4_f32(None, None, 0, None, 0, None, None, None, None, None, 10, 50, 0, 2.0, None, None) == \
        _ffi.MP_OK
    assert lib.mp_acsf_g2_jvp_f32(None, None, 0, None, 0, None, None, None, None, 4, 35, 0, None, None, None) == \
        _ffi.MP_OK
    assert lib.mp_acsf_g4_grad_f32(None, None, 0, None, 0, None, None, None, None, None, None, None, None, None, 10,
                                   50, 0, 2.0, None, None, 0, None, None) == _ffi.MP_OK
    assert lib.mp_relational_dense_f32(None, 0, 640, None, 30, None, None, 35, 6, 0.0, 0, None, None, None, None) == \
        _ffi.MP_OK
    nbytes = ctypes.c_size_t(0)
    assert lib.mp_acsf_grad_ws_bytes(100, 3, ctypes.byref(nbytes)) == _ffi.MP_OK and nbytes.value == 3600
    assert lib.mp_relational_dense_wgrad_ws_bytes(0, 30, ctypes.byref(nbytes)) == _ffi.MP_OK


def _reference_pair_mapping(elements, keep_pair_order):
    """Reference construction (acsf_conv.py:314-340), restated."""
    em = np.array(elements, dtype=int)
    idx = np.expand_dims(em, axis=-1)
    pairs = np.concatenate([np.repeat(np.expand_dims(idx, axis=0), len(em), axis=0),
                            np.repeat(np.expand_dims(idx, axis=1), len(em), axis=1)], axis=-1).reshape((-1, 2))
    if not keep_pair_order:
        pairs = np.sort(pairs, axis=-1)
        pairs = pairs[np.sort(np.unique(pairs, axis=0, return_index=True)[1])]
    return pairs


@pytest.mark.parametrize("elements", [[1, 6, 7, 8], [8, 1, 6], [16, 1]])
def test_param_tables_and_mappings(elements):
    kw2 = ACSFG2.make_param_table(eta=[0.03, 0.5], rs=[0.0, 3.0, 4.0], rc=20.0, elements=elements)
    assert list(kw2["element_mapping"]) == sorted(elements)
    assert kw2["eta_rs_rc"].shape == (len(elements), 6, 3)
    assert np.array_equal(kw2["eta_rs_rc"][0], [[0.03, 0.0, 20.0], [0.5, 0.0, 20.0], [0.03, 3.0, 20.0],
                                                [0.5, 3.0, 20.0], [0.03, 4.0, 20.0], [0.5, 4.0, 20.0]])
    g2 = ACSFG2(**kw2)
    for s, zz in enumerate(sorted(elements)):
        assert g2.reverse_mapping[zz] == s
    assert np.sum(g2.reverse_mapping < np.iinfo(int).max) == len(elements)
    kw4 = ACSFG4.make_param_table(eta=[0.03], zeta=[1.0, 2.0], lamda=[-1.0, 1.0], rc=12.0, elements=elements,
                                  multiplicity=2.0)
    n = len(elements)
    assert kw4["eta_zeta_lambda_rc"].shape == (n * (n + 1) // 2, 4, 4)
    assert np.array_equal(kw4["eta_zeta_lambda_rc"][0], [[0.03, 1.0, -1.0, 12.0], [0.03, 1.0, 1.0, 12.0],
                                                         [0.03, 2.0, -1.0, 12.0], [0.03, 2.0, 1.0, 12.0]])
    g4 = ACSFG4(**kw4)
    assert np.array_equal(g4.element_pair_mapping, _reference_pair_mapping(sorted(elements), False))
    for r, (a, b) in enumerate(g4.element_pair_mapping):
        assert g4.reverse_pair_mapping[a, b] == r and g4.reverse_pair_mapping[b, a] == r
    ordered = ACSFG4(eta_zeta_lambda_rc=np.zeros((n * n, 2, 4)), element_mapping=elements, keep_pair_order=True)
    assert np.array_equal(ordered.element_pair_mapping, _reference_pair_mapping(elements, True))
    for r, (a, b) in enumerate(ordered.element_pair_mapping):
        assert ordered.reverse_pair_mapping[a, b] == r


def test_get_config_keys():
    g2 = ACSFG2(**ACSFG2.make_param_table(eta=[0.1], rs=[0.0], rc=5.0, elements=[1, 6]))
    assert {"eta_rs_rc", "element_mapping", "add_eps", "param_constraint", "param_regularizer", "param_initializer",
            "param_trainable", "name"} <= set(g2.get_config())
    g4 = ACSFG4(**ACSFG4.make_param_table(eta=[0.1], zeta=[1.0], lamda=[1.0], rc=5.0, elements=[1, 6]))
    assert {"eta_zeta_lambda_rc", "add_eps", "element_mapping", "keep_pair_order", "multiplicity",
            "element_pair_mapping", "param_trainable", "param_constraint", "param_regularizer",
            "param_initializer"} <= set(g4.get_config())
    assert {"mean", "std"} <= set(ACSFConstNormalization(std=2.0, mean=1.0).get_config())
    rd = RelationalDense(35, num_relations=30, activation="tanh")
    assert {"units", "use_bias", "num_relations", "num_bases", "num_blocks", "activation", "kernel_initializer",
            "bias_initializer"} <= set(rd.get_config())
    mlp = RelationalMLP(units=[35, 1], num_relations=30, activation=["tanh", "linear"])
    conf = mlp.get_config()
    assert conf["num_relations"] == 30 and conf["units"] == [35, 1] and "num_bases" in conf
    assert ACSFG2._max_atomic_number == 31 and ACSFG4._max_atomic_number == 31


def test_unsupported_options_raise():
    kw = ACSFG2.make_param_table(eta=[0.1], rs=[0.0], rc=5.0, elements=[1, 6])
    with pytest.raises(NotImplementedError):
        ACSFG2(**kw, param_trainable=True)
    with pytest.raises(NotImplementedError):
        ACSFG4(**ACSFG4.make_param_table(eta=[0.1], zeta=[1.0], lamda=[1.0], rc=5.0, elements=[1]),
               param_trainable=True)
    with pytest.raises(NotImplementedError):
        RelationalDense(8, num_relations=4, num_bases=2)
    with pytest.raises(NotImplementedError):
        RelationalDense(8, num_relations=4, num_blocks=2)
    with pytest.raises(NotImplementedError):
        RelationalMLP(units=[8], num_relations=4, use_normalization=True, normalization_technique="graph_batch")
    kwargs = synth.hdnnp_model_kwargs()
    with pytest.raises(NotImplementedError):
        HDNNP2nd.make_model_behler(**dict(kwargs, normalize_kwargs={"epsilon": 1e-3}))
    for fn in (HDNNP2nd.make_model_weighted, HDNNP2nd.make_model_inverse_distances, HDNNP2nd.make_model):
        with pytest.raises(NotImplementedError, match="make_model_behler"):
            fn()


def test_builder_assertions_and_layout():
    kwargs = synth.hdnnp_model_kwargs()
    bad = dict(kwargs, mlp_kwargs=dict(kwargs["mlp_kwargs"], num_relations=8))
    with pytest.raises(AssertionError, match="g2_kwargs"):
        HDNNP2nd.make_model_behler(**bad)
    bad4 = dict(kwargs, g2_kwargs=dict(kwargs["g2_kwargs"], elements=[1, 6]),
                g4_kwargs=dict(kwargs["g4_kwargs"], elements=[1, 6, 40]))
    with pytest.raises(AssertionError, match="g4_kwargs"):
        HDNNP2nd.make_model_behler(**bad4)
    model = HDNNP2nd.make_model_behler(**kwargs)
    shapes = [tuple(t.shape) for _, t in model.weights]
    assert shapes == [(30, 640, 35), (35,), (30, 35, 35), (35,), (30, 35, 1), (1,)]
    assert model.auto_graph is True
    assert HDNNP2nd.make_model is HDNNP2nd.make_model_weighted
    p = synth.hdnnp_params()
    assert [v.shape for v in p.values()] == shapes


def test_synthetic_batch_shape():
    b = synth.hdnnp_batch(num_graphs=2, seed=1)
    assert np.array_equal(np.diff(b["node_splits"]), [22, 22])
    assert set(np.unique(b["node_number"])) == {1, 6, 7, 8}
    assert np.array_equal(np.diff(b["edge_splits"]), [462, 462])
    # every triple (i, j, k) pairs edge (i, j) with an edge (k, j), k != i
    t = b["angle_indices"][:b["angle_splits"][1]]
    assert len(t) == 462 * 20 and np.all(t[:, 2] != t[:, 0]) and np.all(t[:, 2] != t[:, 1])
    assert np.all(np.diff(t[:, 0]) >= 0)
