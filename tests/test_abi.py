"""The C-ABI library loads and exports exactly the symbols that include/mpengine.h, the umbrella over the family headers
of include/mpengine/, declares; the ctypes binding derived from the headers (gcnn_keras_amd/_header.py) is theirs,
literally and against the C compiler; argument errors map to Python exceptions.  No compute is launched (runs without a
GPU)."""
import ctypes
import os
import re
import shutil
import subprocess
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_void_p

import pytest

from gcnn_keras_amd import _ffi, _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    text = re.sub(r"/\*.*?\*/", "", _ffi.HEADER_TEXT, flags=re.S)
    return sorted(set(re.findall(r"\b(mp_[a-z0-9_]+)\s*\(", text)))


def test_library_built_and_loads():
    assert os.path.exists(_ffi.LIB_PATH), "run __graft_entry__.build() first"
    assert _ffi.lib().mp_version() >= 100


def test_every_declared_symbol_is_exported():
    header = _header_symbols()
    assert len(header) >= 30
    assert header == _ffi.declared_symbols(), "ctypes table and header disagree"
    lib = _ffi.lib()
    for name in header:
        assert hasattr(lib, name), name


def test_library_exports_only_what_the_headers_declare():
    """The mp_* names of the dynamic symbol table are the declared ones, no more: a definition without a declaration
    does not compile (-Werror=missing-prototypes), and nothing else may leak out under the prefix."""
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("no nm")
    table = subprocess.run([nm, "-D", "--defined-only", _ffi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = sorted(line.split()[-1] for line in table.splitlines() if line.split()[-1].startswith("mp_"))
    assert exported == _ffi.declared_symbols()


def test_signatures_are_the_headers_literally():
    """Argument lists as the hand-written table had them, one per kind of type the header uses."""
    P, i, i64, f = c_void_p, c_int, c_int64, c_float
    sig = _ffi._SIGNATURES
    assert len(sig) == 198
    assert sig["mp_last_error"] == [] and _ffi._RESTYPES == {"mp_last_error": c_char_p}
    assert sig["mp_cfconv_packed_floats"] == []
    assert sig["mp_device_info"] == [c_char_p, i, P, P]
    assert sig["mp_sort_segments_i32"] == [P, i64, P, P, P, c_size_t, P]
    assert sig["mp_scaler_normal_f64"] == [P, P, i64, P, i, i, P, c_double, i, P, P, P, P, c_size_t, P]
    assert sig["mp_dense_f32"] == [P, i64, i64, P, P, i64, i, f, P, P]
    assert sig["mp_mat_attention_f32"] == [P, i64, P, i64, P, i64, i64, i, i, P, P, i64, P, P, P, P, i64, i, f, f, f, i, P,
                                           i64, i, P, P, P, P]
    assert len(sig["mp_mat_attention_f32"]) == 29
    lib = _ffi.lib()
    assert lib.mp_mat_attention_f32.argtypes == sig["mp_mat_attention_f32"] and lib.mp_last_error.restype is c_char_p
    assert lib.mp_dense_f32.restype is c_int


def test_constants_are_the_headers_literally():
    assert _ffi.MP_EINVAL == -1
    assert _ffi.MP_ACT_LAST == 10          # MP_ACT_LAST = MP_ACT_ELU: an enumerator that names another
    assert _ffi.MP_PAINN_FILTER_IMAGE_BYTES == 73728
    assert _ffi.MP_SCHNET_MAX_DEPTH == 8
    assert _ffi.MP_FLAG_UNKNOWN_SPECIES == 8
    assert _ffi.ACTIVATION_CODES["swish"] == 4 and _ffi.LAYER_ACTIVATION_CODES["elu"] == 10
    from gcnn_keras_amd.autograd import MEGAN_READOUT_SIZES
    assert MEGAN_READOUT_SIZES == {"max_channels": 8, "max_layers": 8, "max_width": 512}


SYNTHETIC = """
#ifndef T_H
#define T_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef void* mpStream_t; /* a comment; with a semicolon */
#define MP_N 3            // and one of the other kind
#define MP_TWICE (2 * MP_N + 0x10)
enum mp_e { MP_A, MP_B, MP_C = MP_N << 2, MP_D, MP_E = -MP_B, MP_F, };
typedef struct mp_inner { const float* p; int32_t a, b; } mp_inner;
typedef struct mp_outer {
  int64_t n;
  const float* w[MP_N]; float* const* q, *r;
  mp_inner in; mp_inner many[2];
  double d; float f[MP_TWICE];
} mp_outer;
const char* mp_name(void);
int mp_go(const mp_outer* desc_host, char* text, int k, int32_t k32, int64_t n, float a, double b, size_t bytes,
          void** out, unsigned long long* counters, mpStream_t stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_on_a_synthetic_header():
    h = _header.parse(SYNTHETIC)
    assert h.constants == {"MP_N": 3, "MP_TWICE": 22, "MP_A": 0, "MP_B": 1, "MP_C": 12, "MP_D": 13, "MP_E": -1, "MP_F": 0}
    assert list(h.structs) == ["mp_inner", "mp_outer"] and list(h.signatures) == ["mp_name", "mp_go"]
    inner, outer = h.structs["mp_inner"], h.structs["mp_outer"]
    assert inner._fields_ == [("p", c_void_p), ("a", c_int), ("b", c_int)]
    fields = dict(outer._fields_)
    assert list(fields) == ["n", "w", "q", "r", "in", "many", "d", "f"]
    assert fields["n"] is c_int64 and fields["q"] is c_void_p and fields["r"] is c_void_p and fields["d"] is c_double
    assert fields["w"]._type_ is c_void_p and fields["w"]._length_ == 3       # sized by a #define
    assert fields["f"]._type_ is c_float and fields["f"]._length_ == 22
    assert fields["in"] is inner                                              # a struct declared earlier, by value
    assert fields["many"]._type_ is inner and fields["many"]._length_ == 2
    assert ctypes.sizeof(outer) == 8 + 3 * 8 + 2 * 8 + 16 + 2 * 16 + 8 + 22 * 4
    assert h.signatures["mp_name"] == [] and h.restypes["mp_name"] is c_char_p
    assert h.signatures["mp_go"] == [c_void_p, c_char_p, c_int, c_int, c_int64, c_float, c_double, c_size_t, c_void_p,
                                     c_void_p, c_void_p]
    assert h.restypes["mp_go"] is c_int


def _write(folder, **files):
    for name, text in files.items():
        (folder / (name + ".h")).write_text(text)
    return str(folder / "all.h")


def test_parser_follows_quoted_includes(tmp_path):
    """An umbrella over two files, the second of which includes the first again: every declaration once, in include
    order, and a constant of the first file sizes a field of the second."""
    (tmp_path / "sub").mkdir()
    umbrella = _write(tmp_path, all='/* umbrella */\n#include <stdint.h>\n#include "sub/a.h"\n  #  include "sub/b.h" /* b */\n')
    _write(tmp_path / "sub",
           a='#ifndef A_H\n#define A_H\n#include <stddef.h>\n#define MP_N 3\ntypedef void* mpStream_t;\n'
             'int mp_first(int a, mpStream_t stream);\n#endif\n',
           b='#ifndef B_H\n#define B_H\n#include "a.h"\ntypedef struct mp_s { float f[MP_N + 1]; } mp_s;\n'
             'int mp_second(const mp_s* desc_host);\n#include "../all.h"\n#endif\n')
    text = _header.expand(umbrella)
    assert text.count("mp_first") == 1 and '#include "' not in text and "#include <stdint.h>" in text
    h = _header.parse(text)
    assert list(h.signatures) == ["mp_first", "mp_second"] and h.constants == {"MP_N": 3}
    assert h.signatures["mp_first"] == [c_int, c_void_p] and h.signatures["mp_second"] == [c_void_p]
    assert ctypes.sizeof(h.structs["mp_s"]) == 16


def test_parser_names_an_include_it_cannot_resolve(tmp_path):
    umbrella = _write(tmp_path, all='#include "here.h"\n#include "sub/missing.h"\n', here="int mp_f(void);\n")
    with pytest.raises(_header.HeaderError) as raised:
        _header.expand(umbrella)
    assert "sub/missing.h" in str(raised.value)
    with pytest.raises(_header.HeaderError) as raised:     # bare text has no folder to look in: expand() comes first
        _header.parse('#include <stdint.h>\n#include "mpengine/core.h"\nint mp_f(void);\n')
    assert "mpengine/core.h" in str(raised.value)


def test_parser_ends_on_headers_that_include_each_other(tmp_path):
    umbrella = _write(tmp_path, all='#include "other.h"\nint mp_a(void);\n#include "all.h"\n',
                      other='#include "all.h"\nint mp_b(void);\n#include "other.h"\n')
    assert list(_header.parse(_header.expand(umbrella)).signatures) == ["mp_b", "mp_a"]


@pytest.mark.parametrize("text, names", [
    ("int mp_f(const float* x, unsigned n);", ["mp_f", "unsigned"]),             # parameter types outside the table
    ("int mp_f(long n);", ["mp_f", "long"]),
    ("int mp_f(mpStream_t stream);", ["mp_f", "mpStream_t"]),                    # a typedef the text does not declare
    ("typedef struct mp_s { int a; } mp_s;\nint mp_f(mp_s by_value);", ["mp_f", "mp_s"]),
    ("int mp_f(const flaot* x);", ["mp_f", "flaot"]),
    ("void mp_f(int a);", ["mp_f", "void"]),                                     # return types other than the two
    ("float mp_f(int a);", ["mp_f", "float"]),
    ("const float* mp_f(int a);", ["mp_f", "float"]),
    ("int mp_f(int (*callback)(int));", ["mp_f"]),                               # declarators it does not understand
    ("int mp_f(float x[3]);", ["mp_f", "x[3]"]),
    ("int mp_f(int64_t, float* out);", ["mp_f", "int64_t"]),
    ("int mp_f(int a, ...);", ["mp_f", "..."]),
    ("typedef struct mp_s { int a : 3; } mp_s;", ["mp_s", "a : 3"]),
    ("typedef struct mp_s { int a, float b; } mp_s;", ["mp_s", "float b"]),
    ("typedef struct mp_s { int (*f)(void); } mp_s;", ["mp_s"]),
    ("typedef struct mp_s { mp_later x; } mp_s;", ["mp_s", "mp_later"]),
    ("typedef struct mp_s { int a[MP_UNKNOWN]; } mp_s;", ["mp_s", "MP_UNKNOWN"]),
    ("typedef struct mp_s { int a; } mp_t;", ["mp_s"]),
    ("typedef int mp_int;", ["mp_int"]),
    ("struct mp_s { int a; };", ["mp_s"]),
    ("enum mp_e { MP_A = 1.5 };", ["mp_e", "MP_A"]),
    ("enum mp_e { MP_A = };", ["mp_e", "MP_A"]),
    ("int mp_f(int a)", ["mp_f"]),                                               # no semicolon
    ("#define MP_X 1.5", ["MP_X"]),                                              # #define MP_* that is no integer
    ("#define MP_X \"text\"", ["MP_X"]),
    ("#define MP_X (MP_Y + 1)", ["MP_X", "MP_Y"]),
    ("#define MP_X", ["MP_X"]),
    ("#define MP_X(a) (a)", ["MP_X"]),
    ("#define MP_X 1 2", ["MP_X"]),
    ("#define MP_X 1 / 0", ["MP_X"]),
    ("#define OTHER 1", ["OTHER"]),
    ("#if 0\nint mp_f(int a);\n#endif", ["#if 0"]),                              # would be bound although it is dead
])
def test_parser_refuses_what_it_does_not_understand(text, names):
    with pytest.raises(_header.HeaderError) as raised:
        _header.parse(text)
    for name in names:
        assert name in str(raised.value), str(raised.value)


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """sizeof and every offsetof of the nine descriptor structs, host cc against ctypes (the umbrella compiles as C)."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no host C compiler")
    structs = _ffi._ABI.structs
    assert len(structs) == 9
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "mpengine.h"', "int main(void) {"]
    expected = []
    for name, cls in structs.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        expected.append("%s %d" % (name, ctypes.sizeof(cls)))
        for field, _ in cls._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, field, name, field))
            expected.append("%s.%s %d" % (name, field, getattr(cls, field).offset))
    source, program = tmp_path / "layout.c", tmp_path / "layout"
    source.write_text("\n".join(lines + ["  return 0;", "}"]) + "\n")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(program),
                    str(source)], check=True)
    printed = subprocess.run([str(program)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert printed[:-1] == expected
    assert ctypes.sizeof(_ffi.SchnetForwardDesc) == 744 and ctypes.sizeof(_ffi.SchnetForceDesc) == 1160


def test_argument_errors_map_to_python_exceptions():
    lib = _ffi.lib()
    rc = lib.mp_dense_f32(None, 4, 0, None, None, 4, 0, 0.0, None, None)
    assert rc == _ffi.MP_EINVAL
    with pytest.raises(ValueError):
        _ffi.check(rc)
    assert b"mp_dense_f32" in lib.mp_last_error()
    rc = lib.mp_segment_reduce_csr_f32(9, None, 0, 1, None, None, 0, None, 0, None, None)
    assert rc == _ffi.MP_EINVAL
    # the SchNet node chains read packed weight images only: flags bit 1 clear is refused before the pointers are looked at
    for name, call in (
            ("mp_schnet_node_in_f32", lambda: lib.mp_schnet_node_in_f32(None, 4, None, 10, 64, None, None, None, None, None,
                                                                        1, None)),
            ("mp_schnet_node_update_f32", lambda: lib.mp_schnet_node_update_f32(None, 4, None, None, None, None, None, None,
                                                                                None, 1, None)),
            ("mp_schnet_node_last_f32", lambda: lib.mp_schnet_node_last_f32(None, 4, None, None, None, None, None, None, None,
                                                                            None, None, None, 1, None))):
        assert call() == _ffi.MP_EINVAL
        message = lib.mp_last_error()
        assert name.encode() in message and b"flags bit 1" in message
    # zero-sized problems are accepted without touching the device
    assert lib.mp_gather_rows_f32(None, 0, 4, None, 0, 1, _ffi.int32_array([0]), None, None) == _ffi.MP_OK
    assert lib.mp_shift_index_i64(None, 0, 2, None, None, 0, 1, None, None) == _ffi.MP_OK


def test_no_cpu_fallback():
    import torch
    from gcnn_keras_amd.layers.modules import dense_values
    with pytest.raises(_ffi.EngineError):
        dense_values(torch.zeros(2, 3), torch.zeros(3, 4), None)
