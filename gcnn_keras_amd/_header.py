"""Strict parser of include/mpengine.h and the family headers it includes: they are the one declaration of the C ABI,
``_ffi`` derives its ctypes tables from them.

``expand(path)`` gives a header's text with every quoted ``#include`` replaced by the text of that file; ``parse(text)``
understands exactly what the header uses - ``#define MP_*`` integer constants, ``enum``s, a ``typedef``
of a pointer, ``typedef struct name { ... } name;`` and prototypes returning ``int`` or ``const char*`` - and raises
``HeaderError`` naming the declaration for anything else: a wrong guess here would hand a kernel a wrong device pointer.
"""
import collections
import ctypes
import os
import re

# C type -> ctypes type of a parameter or field.  Every pointer is c_void_p, except a char* parameter (c_char_p).
SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
           "double": ctypes.c_double, "size_t": ctypes.c_size_t}
_POINTEES = set(SCALARS) | {"void", "char", "unsigned long long"}   # what a pointer may point to, besides a struct

Header = collections.namedtuple("Header", "constants structs signatures restypes")


class HeaderError(ValueError):
    pass


_NAME = r"[A-Za-z_]\w*"
_DECLARATION = re.compile(r"(#[^\n]*|[^;{}#]*(?:\{[^{}]*\}[^;{}#]*)?;)\s*")   # a directive line, or up to the next ';'
_DEFINE = re.compile(r"#\s*define\s+(%s)\b(.*)" % _NAME)
_BLOCK = re.compile(r"(enum|typedef struct)\s+(%s)\s*\{(.*)\}\s*(\w*)" % _NAME)
_PROTOTYPE = re.compile(r"([^()]+)\(([^()]*)\)")
_DECLARATOR = re.compile(r"\s*(?:((?:%s\s+)*%s)(?=[\s*]))?\s*((?:\*\s*)*)(%s)\s*(?:\[([^\][]*)\])?\s*"
                         % (_NAME, _NAME, _NAME))
_QUOTED_INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]*"([^"\n]*)"[^\n]*$', re.M)
_EXPR_TOKEN = re.compile(r"0[xX][0-9a-fA-F]+|\d+|(%s)|<<|>>|[-+*/%%|&^~()]" % _NAME)


def expand(path, seen=None):
    """Text of the header ``path`` with every line ``#include "x.h"`` replaced by the text of x.h, looked up beside the
    including file.  A file is read once: a repeated include, or one that closes a cycle, expands to nothing."""
    seen = set() if seen is None else seen
    if os.path.realpath(path) in seen:
        return ""
    seen.add(os.path.realpath(path))
    with open(path) as file:
        text = file.read()

    def included(found):
        target = os.path.join(os.path.dirname(path), found.group(1))
        if not os.path.isfile(target):
            raise HeaderError('%s: #include "%s": no such file' % (path, found.group(1)))
        return expand(target, seen)
    return _QUOTED_INCLUDE.sub(included, text)


def _integer(expr, constants, where):
    """Value of an integer expression over literals and the constants declared so far."""
    def python(token):
        name = token.group(1)
        if name is None:
            return token.group().replace("/", "//")
        if name not in constants:
            raise HeaderError("%s: %r is not an integer constant declared before it" % (where, name))
        return "(%d)" % constants[name]
    code = _EXPR_TOKEN.sub(python, expr)
    try:
        if _EXPR_TOKEN.sub("", expr).strip():
            raise SyntaxError(expr)
        return int(eval(code, {"__builtins__": {}}))
    except Exception:
        raise HeaderError("%s: cannot evaluate %r to an integer" % (where, expr.strip())) from None


def _declarator(text, where):
    """``type *... name [size]`` -> (type, pointer levels, name, size text or None).  The type is None in the
    second and later declarators of one declaration."""
    found = _DECLARATOR.fullmatch(text)
    if not found:
        raise HeaderError("%s: declarator %r not understood" % (where, text.strip()))
    kind, stars, name, size = found.groups()
    return kind, stars.count("*"), name, size


def _ctype(kind, stars, ctype_of, structs, owner, member, by_value=False):
    """ctypes type of ``member`` (a field, parameter or typedef) of ``owner``; ``by_value`` admits a struct that is not
    behind a pointer."""
    if stars:
        if kind not in _POINTEES and kind not in ctype_of and kind not in structs:
            raise HeaderError("%s: %s: pointer to unknown type %r" % (owner, member, kind))
        return ctypes.c_void_p
    if kind in ctype_of:
        return ctype_of[kind]
    if by_value and kind in structs:
        return structs[kind]
    raise HeaderError("%s: %s: type %r is outside the binding's type table" % (owner, member, kind))


def _enum(name, body, constants):
    value = -1
    for item in filter(None, (i.strip() for i in body.split(","))):
        enumerator, eq, expr = (s.strip() for s in item.partition("="))
        if not re.fullmatch(_NAME, enumerator):
            raise HeaderError("enum %s: enumerator %r not understood" % (name, item))
        value = _integer(expr, constants, "enum %s: %s" % (name, enumerator)) if eq else value + 1
        constants[enumerator] = value


def _struct(name, body, constants, ctype_of, structs):
    fields = []
    for member in filter(None, (m.strip() for m in body.split(";"))):
        for i, piece in enumerate(member.split(",")):
            words, stars, field, size = _declarator(piece, "struct " + name)
            if bool(words) != (i == 0):   # one type, in front of the first declarator
                raise HeaderError("struct %s: declarator %r not understood" % (name, piece.strip()))
            kind = words or kind
            ctype = _ctype(kind, stars, ctype_of, structs, "struct " + name, field, by_value=True)
            if size is not None:
                ctype = ctype * _integer(size, constants, "struct %s: %s" % (name, field))
            fields.append((field, ctype))
    return type(name, (ctypes.Structure,), {"_fields_": fields})


def _prototype(decl, ctype_of, structs):
    found = _PROTOTYPE.fullmatch(decl)
    if not found:
        raise HeaderError("declaration %r not understood" % decl[:80])
    kind, stars, name, size = _declarator(found.group(1), decl[:80])
    restype = {("int", 0): ctypes.c_int, ("char", 1): ctypes.c_char_p}.get((kind, stars))
    if restype is None or size is not None:
        raise HeaderError("%s: return type %r is neither int nor const char*" % (name, "%s%s" % (kind, "*" * stars)))
    argtypes = []
    if found.group(2).strip() != "void":
        for param in found.group(2).split(","):
            kind, stars, pname, size = _declarator(param, name)
            if kind is None or size is not None:
                raise HeaderError("%s: parameter %r needs a type and a name, and no array" % (name, param.strip()))
            ctype = _ctype(kind, stars, ctype_of, structs, name, pname)
            argtypes.append(ctypes.c_char_p if (kind, stars) == ("char", 1) else ctype)
    return name, argtypes, restype


def parse(text):
    """``Header(constants, structs, signatures, restypes)`` of a header text, each a dict by name in header order:
    integer values, ``ctypes.Structure`` classes, argtypes lists and restypes."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*|\bconst\b", " ", text, flags=re.S)   # comments; const changes no ctypes type
    text = re.sub(r"#\s*ifdef\s+__cplusplus\b.*?#\s*endif", " ", text, flags=re.S).strip()   # extern "C" { and }
    constants, structs, signatures, restypes = {}, {}, {}, {}
    ctype_of = dict(SCALARS)   # grows by the header's own pointer typedefs (mpStream_t)
    pos = 0
    while pos < len(text):
        found = _DECLARATION.match(text, pos)
        if not found:
            raise HeaderError("cannot split a declaration off %r" % text[pos:pos + 60])
        pos = found.end()
        decl = " ".join(found.group(1).rstrip(";").split())
        define, block = _DEFINE.fullmatch(decl), _BLOCK.fullmatch(decl)
        if define and define.group(1).startswith("MP_"):
            constants[define.group(1)] = _integer(define.group(2), constants, "#define " + define.group(1))
        elif define and define.group(2).strip():
            raise HeaderError("%r: only MP_* integer constants are bound" % decl)
        elif decl.startswith("#"):   # include guards and #include <...> pass; a conditional section would be read as live
            if not re.match(r"#\s*(include\s*<|ifndef\b|define\b|endif\b)", decl):   # #include "x.h": expand() comes first
                raise HeaderError("%r: directive not understood" % decl)
        elif block and block.group(1) == "enum" and not block.group(4):
            _enum(block.group(2), block.group(3), constants)
        elif block and block.group(1) == "typedef struct" and block.group(4) == block.group(2):
            structs[block.group(2)] = _struct(block.group(2), block.group(3), constants, ctype_of, structs)
        elif decl.startswith("typedef ") and not block:
            kind, stars, name, size = _declarator(decl[len("typedef "):], decl)
            if not stars or size is not None:
                raise HeaderError("%r: only a typedef of a pointer or of a struct is understood" % decl)
            ctype_of[name] = _ctype(kind, stars, ctype_of, structs, decl, name)
        elif block:
            raise HeaderError("declaration %r not understood" % decl[:80])
        else:
            name, signatures[name], restypes[name] = _prototype(decl, ctype_of, structs)
    return Header(constants, structs, signatures, restypes)
