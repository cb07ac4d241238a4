"""ctypes binding of libmpengine.so (the C ABI declared in include/mpengine.h).

This is the only place where Python meets the engine: plain pointers and sizes cross the boundary, torch is used
for device memory and streams only.  There is NO CPU fallback: if the shared library is missing or a tensor is
not on a HIP device, the call fails loudly.

Nothing of the ABI is written down here.  The umbrella header and the family headers it includes (include/mpengine/*.h),
and behind them the family headers of ``PENDING_HEADERS``, are read once at import (``_header.expand`` and
``_header.parse``, strict: a declaration it does not understand is an error) and give every ``MP_*`` constant as a
module attribute, the descriptor structs as ``ctypes.Structure`` classes and the argument and return types of every
entry point.  A new entry point is declared in a family header and defined in csrc/, nowhere else.
"""
import ctypes
import os
from ctypes import c_char_p, c_int, c_int64, c_size_t, c_void_p

import torch

from . import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libmpengine.so")
HEADER_PATH = os.path.join(_HERE, "..", "include", "mpengine.h")   # the umbrella over include/mpengine/*.h

# Family headers that wait for their #include line in the umbrella: read behind it with the same parser (their core.h is
# the umbrella's, expanded once), their prototypes kept in a table of their own.  A header leaves this tuple when the
# umbrella includes it; its prototypes then count among ``_SIGNATURES``.
PENDING_HEADERS = ("mpengine/inorp.h",)
# Family headers that came after it and wait the same way, read behind the pending ones; their prototypes are kept apart
# in ``_FAMILY_SIGNATURES``: tests/test_inorp_api.py pins ``PENDING_HEADERS`` and ``_PENDING_SIGNATURES`` to INorp's own.
FAMILY_HEADERS = ("mpengine/mxmnet.h",)

_seen = set()
_UMBRELLA_TEXT = _header.expand(HEADER_PATH, _seen)   # the umbrella with every family header in place of its #include
_PENDING_TEXT = _UMBRELLA_TEXT + "".join(
    "\n" + _header.expand(os.path.join(os.path.dirname(HEADER_PATH), _name), _seen) for _name in PENDING_HEADERS)
_FAMILY_TEXTS = {_name: _header.expand(os.path.join(os.path.dirname(HEADER_PATH), _name), _seen)
                 for _name in FAMILY_HEADERS}
HEADER_TEXT = _PENDING_TEXT + "".join("\n" + _text for _text in _FAMILY_TEXTS.values())
_ABI = _header.parse(_UMBRELLA_TEXT)
_PENDING_ABI = _header.parse(_PENDING_TEXT)
_FULL_ABI = _header.parse(HEADER_TEXT)

globals().update(_FULL_ABI.constants)   # MP_OK, MP_EINVAL, MP_SUM, MP_ACT_*, MP_SCHNET_MAX_DEPTH, ...: every constant
_SIGNATURES = _ABI.signatures      # name -> argtypes, of the umbrella
_PENDING_SIGNATURES = {name: args for name, args in _PENDING_ABI.signatures.items() if name not in _SIGNATURES}
_FAMILY_SIGNATURES = {name: args for name, args in _FULL_ABI.signatures.items()
                      if name not in _SIGNATURES and name not in _PENDING_SIGNATURES}
_RESTYPES = {name: restype for name, restype in _FULL_ABI.restypes.items() if restype is not c_int}   # int unless listed

FilterTableLayout = _ABI.structs["mp_filter_table_layout"]
SchnetForwardDesc = _ABI.structs["mp_schnet_forward_desc"]
SchnetForceDesc = _ABI.structs["mp_schnet_force_desc"]
BatchSrc = _ABI.structs["mp_batch_src"]
ConcatDesc = _ABI.structs["mp_concat_desc"]
TakeItem = _ABI.structs["mp_take_item"]
TakeDesc = _ABI.structs["mp_take_desc"]
GcnLayerDesc = _ABI.structs["mp_gcn_layer"]
GcnTileDesc = _ABI.structs["mp_gcn_tile_desc"]

ACTIVATION_CODES = {
    None: MP_ACT_LINEAR, "linear": MP_ACT_LINEAR, "relu": MP_ACT_RELU,
    "kgcnn>shifted_softplus": MP_ACT_SHIFTED_SOFTPLUS, "shifted_softplus": MP_ACT_SHIFTED_SOFTPLUS,
    "softplus": MP_ACT_SOFTPLUS, "swish": MP_ACT_SWISH, "sigmoid": MP_ACT_SIGMOID, "tanh": MP_ACT_TANH,
    "kgcnn>leaky_relu": MP_ACT_LEAKY_RELU, "leaky_relu": MP_ACT_LEAKY_RELU,
    "kgcnn>softplus2": MP_ACT_SOFTPLUS2, "softplus2": MP_ACT_SOFTPLUS2, "selu": MP_ACT_SELU, "kgcnn>swish": MP_ACT_SWISH,
}
# ACTIVATION_CODES is the set the fused routes' `*_supported` decisions are taken on; LAYER_ACTIVATION_CODES is what the
# Dense / Activation layers and their reverse rules run (``activation_code``): additionally Keras "elu", AttentiveFP's
# context activation, which only csrc/mp_attentivefp.hip takes among the fused kernels.
LAYER_ACTIVATION_CODES = dict(ACTIVATION_CODES, elu=MP_ACT_ELU)

_lib = None


class EngineError(RuntimeError):
    pass


def declared_symbols():
    """Names of every entry point declared under include/mpengine.h and in the headers of ``PENDING_HEADERS`` and
    ``FAMILY_HEADERS`` (checked by tests/test_abi.py)."""
    return sorted(list(_SIGNATURES) + list(_PENDING_SIGNATURES) + list(_FAMILY_SIGNATURES))


def lib():
    """Load libmpengine.so once.  Raises if it was not built (run ``python -c 'import __graft_entry__ as g; g.build()'``).
    ``MPENGINE_LIB`` names another build of the same ABI - used by ``make -C gcnn_keras_amd/csrc asan``, whose
    host-only AddressSanitizer build exports the host packer and runtime entry points only (missing kernels are then
    simply not bound; calling one raises AttributeError)."""
    global _lib
    if _lib is None:
        path = os.environ.get("MPENGINE_LIB") or LIB_PATH
        if not os.path.exists(path):
            raise EngineError("libmpengine.so not found at %s - build it with __graft_entry__.build() "
                              "(there is no CPU fallback)" % path)
        handle = ctypes.CDLL(path)
        for name, argtypes in (list(_SIGNATURES.items()) + list(_PENDING_SIGNATURES.items())
                               + list(_FAMILY_SIGNATURES.items())):
            fn = getattr(handle, name, None)
            if fn is None:
                if path == LIB_PATH:
                    raise EngineError("libmpengine.so lacks %s - rebuild it (__graft_entry__.build())" % name)
                continue
            fn.argtypes = argtypes
            fn.restype = _RESTYPES.get(name, c_int)
        _lib = handle
    return _lib


def check(rc):
    if rc == MP_OK:
        return
    msg = lib().mp_last_error().decode("utf-8", "replace")
    if rc == MP_EINVAL:
        raise ValueError(msg)
    if rc == MP_EINDEX:
        raise IndexError(msg)
    raise EngineError("libmpengine status %d: %s" % (rc, msg))


def require_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise EngineError("gcnn_keras_amd ops run on an MI355X only: got a %s tensor (no CPU fallback)" % t.device)


def ptr(t):
    """Device pointer of a contiguous torch tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_contiguous():
        raise ValueError("engine buffers must be contiguous")
    return c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def stream_handle():
    """Integer hipStream_t of torch's current stream.  ``torch.cuda.current_stream().cuda_stream`` builds a Stream object
    and resolves the device index through several Python layers (~5 us, three times per model call before); the two C
    entry points underneath it take ~0.3 us."""
    if _raw_stream is not None and _raw_device is not None:
        return _raw_stream(_raw_device())
    return torch.cuda.current_stream().cuda_stream


def stream():
    """hipStream_t of torch's current stream (torch is plumbing: memory + streams)."""
    return c_void_p(stream_handle())


_has_gpu = None


def has_gpu():
    """``torch.cuda.is_available()`` once per process (the call reads environment variables every time)."""
    global _has_gpu
    if _has_gpu is None:
        _has_gpu = bool(torch.cuda.is_available())
    return _has_gpu


_launches = [0]


def launch_count():
    """Number of engine calls issued so far by this process (bench.py reports calls per forward)."""
    return _launches[0]


_roctx = None


def enable_roctx(on=True):
    """Bracket every engine call in a roctx range named after the entry point (``rocprofv3 --marker-trace`` then shows
    which C-ABI call a kernel belongs to).  Also switched on by ``MPENGINE_ROCTX=1``.  Off by default: two extra
    library calls per launch."""
    global _roctx
    if not on:
        _roctx = None
        return
    for cand in ("libroctx64.so", "/opt/rocm/lib/libroctx64.so", "librocprofiler-sdk-roctx.so",
                 "/opt/rocm/lib/librocprofiler-sdk-roctx.so"):
        try:
            h = ctypes.CDLL(cand)
            h.roctxRangePushA.argtypes = [c_char_p]
            h.roctxRangePushA.restype = c_int
            h.roctxRangePop.restype = c_int
            _roctx = h
            return
        except (OSError, AttributeError):
            continue
    raise EngineError("no roctx library found under /opt/rocm/lib")


def call(name, *args):
    _launches[0] += 1
    if _roctx is not None:
        _roctx.roctxRangePushA(name.encode())
        try:
            check(getattr(lib(), name)(*args))
        finally:
            _roctx.roctxRangePop()
        return
    check(getattr(lib(), name)(*args))


def workspace_bytes(name, *args):
    """Size in bytes that the query entry point ``name`` (``mp_*_ws_bytes`` / ``mp_*_workspace_bytes``) reports for
    ``args``: one engine call, its ``size_t*`` result as an int."""
    nbytes = c_size_t(0)
    call(name, *args, ctypes.byref(nbytes))
    return nbytes.value


def float_workspace(name, *args, device, none_if_empty=False):
    """``(ws, nbytes)``: a float32 workspace of ``workspace_bytes(name, *args)`` bytes and that size.  0 bytes give one
    element, so that ``ws`` has a pointer, or ``None`` with ``none_if_empty``."""
    nbytes = workspace_bytes(name, *args)
    if none_if_empty and not nbytes:
        return None, 0
    return torch.empty((max(nbytes, 4) // 4,), dtype=torch.float32, device=device), nbytes


if os.environ.get("MPENGINE_ROCTX") == "1":
    try:
        enable_roctx()
    except EngineError:
        pass


def activation_code(name):
    if isinstance(name, dict):
        name = name.get("class_name", name.get("name"))
    if name not in LAYER_ACTIVATION_CODES:
        raise ValueError("Activation %r is not supported by the engine" % (name,))
    return LAYER_ACTIVATION_CODES[name]


def int64_array(values):
    return (c_int64 * len(values))(*values)


def int32_array(values):
    return (ctypes.c_int32 * len(values))(*values)
