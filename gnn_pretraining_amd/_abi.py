"""The C ABI of libgnnmp.so, read from include/gnnmp.h and include/gnnmp_step.h: the headers are the only place a
constant, a struct or a prototype is written down.  parse() turns header text into ctypes; whatever it does not
recognise raises GnnmpError quoting the declaration, it never guesses a type.

`python -m gnn_pretraining_amd._abi > tests/golden/abi_snapshot.json` rewrites the snapshot tests/test_layout.py pins."""
from __future__ import annotations

import ast
import ctypes as C
import json
import operator
import os
import re
from types import SimpleNamespace

_INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADER_PATH = os.path.join(_INCLUDE, "gnnmp.h")
STEP_HEADER_PATH = os.path.join(_INCLUDE, "gnnmp_step.h")


class GnnmpError(RuntimeError):
    pass


SCALARS = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
           "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "gmp_stream_t": C.c_void_p}
POINTEES = ("void", "char", "uint8_t")      # known, but only behind a star
_OPS = {ast.Add: operator.add, ast.Sub: operator.sub, ast.Mult: operator.mul}
_DECLARATOR = r"((?:\*\s*)*)(\w+)?\s*(\[[^\[\]]*\])?"


def _value(expr: str, consts: dict, decl: str) -> int:
    """An integer expression of + - * ( ) over literals and earlier constants."""
    def ev(n):
        if isinstance(n, ast.Constant) and type(n.value) is int:
            return n.value
        if isinstance(n, ast.Name) and n.id in consts:
            return consts[n.id]
        if isinstance(n, ast.BinOp) and type(n.op) in _OPS:
            return _OPS[type(n.op)](ev(n.left), ev(n.right))
        if isinstance(n, ast.UnaryOp) and isinstance(n.op, ast.USub):
            return -ev(n.operand)
        raise GnnmpError(f"cannot evaluate the constant `{expr.strip()}` in `{decl}`")
    try:
        return ev(ast.parse(expr.strip(), mode="eval").body)
    except SyntaxError:
        raise GnnmpError(f"cannot evaluate the constant `{expr.strip()}` in `{decl}`") from None


def _ctype(base: str, stars: int, structs: dict, decl: str, where: str):
    """ctypes of `base` behind `stars` stars; where = "field", "arg" or "ret"."""
    if not (base in SCALARS or base in structs or (base in POINTEES and stars) or (base, stars, where) == ("void", 0, "ret")):
        raise GnnmpError(f"unknown type `{base}` in `{decl}`")
    if stars:
        if stars == 1 and base in structs and where != "field":
            return C.POINTER(structs[base])
        return C.c_char_p if (base, stars, where) == ("char", 1, "ret") else C.c_void_p
    if base in SCALARS:
        return SCALARS[base]
    if base == "void":
        return None
    return structs[base] if where == "field" else _bad(decl)      # a struct by value is a member, never an argument


def _bad(decl: str):
    raise GnnmpError(f"cannot parse the declaration `{decl}`")


def _fields(body: str, consts: dict, structs: dict) -> list:
    out = []
    for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
        m = re.fullmatch(r"(\w+)\s*(.+)", re.sub(r"\bconst\b", " ", decl).strip()) or _bad(decl)
        for one in m.group(2).split(","):
            d = re.fullmatch(_DECLARATOR, one.strip())
            if not d or not d.group(2):
                _bad(decl)
            t = _ctype(m.group(1), d.group(1).count("*"), structs, decl, "field")
            out.append((d.group(2), t * _value(d.group(3)[1:-1], consts, decl) if d.group(3) else t))
    return out


def _function(decl: str, structs: dict):
    m = re.fullmatch(r"(\w+)\s*((?:\*\s*)*)(\w+)\s*\((.*)\)", re.sub(r"\bconst\b", " ", decl).strip()) or _bad(decl)
    args = []
    for one in ([] if m.group(4).strip() == "void" else m.group(4).split(",")):
        a = re.fullmatch(r"(\w+)\s*" + _DECLARATOR, one.strip()) or _bad(decl)
        if a.group(4) not in (None, "[]"):
            _bad(decl)
        args.append(_ctype(a.group(1), a.group(2).count("*") + bool(a.group(4)), structs, decl, "arg"))
    return m.group(3), (_ctype(m.group(1), m.group(2).count("*"), structs, decl, "ret"), args)


def parse(*headers: str) -> SimpleNamespace:
    """constants {name: int}, structs {C name: ctypes.Structure subclass} and functions {name: (restype, [argtypes])}
    of the given header texts, each in header order."""
    consts, structs, functions = {}, {}, {}
    for text in headers:
        text = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
        for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S.*)$|\benum\s*\{([^{}]*)\}\s*;", text, flags=re.M):
            if m.group(1):
                consts[m.group(1)] = _value(m.group(2), consts, m.group(0).strip())
                continue
            nxt = 0
            for e in filter(None, (e.strip() for e in m.group(3).split(","))):
                name, _, expr = (s.strip() for s in e.partition("="))
                consts[name] = nxt = _value(expr, consts, e) if expr else nxt
                nxt += 1
        text = re.sub(r"^[ \t]*#.*$|\benum\s*\{[^{}]*\}\s*;|\btypedef\s+void\s*\*\s*gmp_stream_t\s*;|\bextern\s+\"C\"\s*\{", " ", text, flags=re.M)

        def struct(m):
            structs[m.group(2)] = type(m.group(2), (C.Structure,), {"_fields_": _fields(m.group(1), consts, structs)})
            return " "
        *decls, tail = re.sub(r"\btypedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text).split(";")
        if tail.strip() not in ("", "}"):       # "}" closes extern "C"
            _bad(" ".join(tail.split()))
        for decl in filter(None, (" ".join(d.split()) for d in decls)):
            name, sig = _function(decl, structs)
            functions[name] = sig
    return SimpleNamespace(constants=consts, structs=structs, functions=functions)


def load() -> SimpleNamespace:
    return parse(open(HEADER_PATH).read(), open(STEP_HEADER_PATH).read())


def _name(t) -> str:
    return "None" if t is None else f"POINTER({t._type_.__name__})" if hasattr(t, "contents") else t.__name__


def snapshot(abi: SimpleNamespace) -> dict:
    """What crosses the boundary, as plain data: the constants Python uses, every function's type names and every
    struct's [field, offset, size] rows and total size."""
    return {
        "constants": {k: v for k, v in abi.constants.items() if re.match(r"GMP_(STEP_(MAX_|LAYERS)|TASK_|SURGERY_|GEMM_)", k)},
        "functions": {k: [_name(r), [_name(a) for a in args]] for k, (r, args) in abi.functions.items()},
        "structs": {k: {"size": C.sizeof(s), "fields": [[f, getattr(s, f).offset, getattr(s, f).size] for f, _ in s._fields_]}
                    for k, s in abi.structs.items()},
    }


if __name__ == "__main__":
    print(json.dumps(snapshot(load()), indent=1, sort_keys=True))
