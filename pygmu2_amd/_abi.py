"""
Strict reader of include/pygmu_hip.h, the one definition of the library's C ABI: every prototype as ctypes classes,
every parameter struct as a packed numpy dtype, every PGX_* constant.  Inside the header's extern "C" block a
statement is a #define, the status enum, a typedef struct, a second name for an earlier struct (`typedef pgx_a pgx_b;`:
the same type to the compiler, the same dtype here, no table entry of its own) or a prototype; anything else, and any
type name not listed here, raises AbiError with its line -- a declaration is never skipped.
"""

from __future__ import annotations

import ast
import ctypes as C
import re

import numpy as np


class AbiError(ValueError):
    pass


_SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double, "float": C.c_float, "size_t": C.c_size_t,
            "uint64_t": C.c_uint64}
_POINTEES = {"void", "char", "int16_t", "int32_t"}          # read only behind a pointer
_FIELDS = {"double": "<f8", "float": "<f4", "int": "<i4", "int32_t": "<i4", "int64_t": "<i8", "uint64_t": "<u8"}

_BLOCK = re.compile(r'#ifdef __cplusplus\s*extern "C" \{\s*#endif(.*)#ifdef __cplusplus\s*\}\s*#endif', re.S)
_SPACE = re.compile(r"\s*")
_DEFINE = re.compile(r"#define[ \t]+(PGX_\w+)[ \t]+(.*)")
_ENUM = re.compile(r"typedef\s+enum\s*\{([^{}]*)\}\s*pgx_\w+\s*;")
_STRUCT = re.compile(r"typedef\s+struct\s*\{([^{}]*)\}\s*(pgx_\w+)\s*;")
_ALIAS = re.compile(r"typedef\s+(pgx_\w+)\s+(pgx_\w+)\s*;")
_PROTOTYPE = re.compile(r"([^;{}#()]+)\(([^;{}#()]*)\)\s*;")
# [PGX_HOST] [const] type [* [const]]... name [[N]]
_DECLARATION = re.compile(r"(PGX_HOST\s+)?(?:const\s+)?(\w+)\s*((?:\*\s*(?:const\s*)?)*)\b(\w+)\s*(?:\[(\d*)\])?")
_DECLARATOR = re.compile(r"(\**)\s*(\w+)\s*(?:\[(\d+)\])?")


class Abi:
    def __init__(self):
        self.functions = {}        # name -> (restype, [argtypes]), header order
        self.structs = {}          # pgx_name -> np.dtype
        self.aliases = {}          # pgx_name -> the pgx_name of the struct it is another name for
        self.constants = {}        # PGX_NAME -> int | float

    def struct(self, name: str) -> np.dtype:
        name = self.aliases.get(name, name)
        if name not in self.structs:
            raise AbiError(f"pygmu_hip.h declares no struct {name}")
        return self.structs[name]

    def constant(self, name: str):
        if name not in self.constants:
            raise AbiError(f"pygmu_hip.h defines no constant {name}")
        return self.constants[name]


def _evaluate(expr: str, names: dict, line: int):
    """Literals, earlier constants and + - * / (C's: truncating between integers), by a walk over the syntax tree."""
    def walk(node):
        if isinstance(node, ast.Constant) and type(node.value) in (int, float):
            return node.value
        if isinstance(node, ast.Name) and node.id in names:
            return names[node.id]
        if isinstance(node, ast.UnaryOp) and isinstance(node.op, (ast.USub, ast.UAdd)):
            return -walk(node.operand) if isinstance(node.op, ast.USub) else walk(node.operand)
        if isinstance(node, ast.BinOp) and isinstance(node.op, (ast.Add, ast.Sub, ast.Mult, ast.Div)):
            a, b = walk(node.left), walk(node.right)
            if isinstance(node.op, ast.Div):
                exact = isinstance(a, int) and isinstance(b, int)
                return abs(a) // abs(b) * (1 if (a < 0) == (b < 0) else -1) if exact else a / b
            return a + b if isinstance(node.op, ast.Add) else a - b if isinstance(node.op, ast.Sub) else a * b
        raise AbiError(f"pygmu_hip.h:{line}: cannot evaluate {expr.strip()!r}")
    try:
        return walk(ast.parse(expr.strip(), mode="eval").body)
    except (SyntaxError, ZeroDivisionError):
        raise AbiError(f"pygmu_hip.h:{line}: cannot evaluate {expr.strip()!r}") from None


def _ctype(text: str, structs: dict, line: int, returned: bool = False):
    """One parameter (or `type name` of a return value) -> (ctypes class, name)."""
    m = _DECLARATION.fullmatch(" ".join(text.split()))
    if not m:
        raise AbiError(f"pygmu_hip.h:{line}: cannot read the declaration {text.strip()!r}")
    host, base, stars, name, array = m.groups()
    depth = stars.count("*") + (array is not None)
    if base not in _SCALARS and not (depth and (base in _POINTEES or base in structs)):
        raise AbiError(f"pygmu_hip.h:{line}: unknown type {base!r} in {text.strip()!r}")
    if depth == 0:
        return _SCALARS[base], name
    if base == "char" and depth == 1 and (host or returned):
        return C.c_char_p, name
    if not host:
        return C.c_void_p, name                              # a device pointer, passed as an integer
    if depth == 2:
        return C.POINTER(C.c_void_p), name
    if depth > 2 or base not in _SCALARS:
        raise AbiError(f"pygmu_hip.h:{line}: PGX_HOST cannot describe {text.strip()!r}")
    return C.POINTER(_SCALARS[base]), name


def _dtype(body: str, structs: dict, line: int) -> np.dtype:
    fields = []
    *declarations, rest = body.split(";")
    if rest.strip():
        raise AbiError(f"pygmu_hip.h:{line + body.count(chr(10))}: field without ';': {rest.strip()!r}")
    for text in declarations:
        at = line + text[:len(text) - len(text.lstrip())].count("\n")
        line += text.count("\n")
        m = re.fullmatch(r"(?:const\s+)?(\w+)\b(.*)", text.strip(), re.S)
        base = m.group(1) if m else None
        if base not in _FIELDS and base not in _POINTEES and base not in structs:
            raise AbiError(f"pygmu_hip.h:{at}: cannot read the field {text.strip()!r}")
        for declarator in m.group(2).split(","):
            d = _DECLARATOR.fullmatch(declarator.strip())
            if not d or (not d.group(1) and base not in _FIELDS):
                raise AbiError(f"pygmu_hip.h:{at}: cannot read the field {text.strip()!r}")
            kind = "<u8" if d.group(1) else _FIELDS[base]
            fields.append((d.group(2), kind, (int(d.group(3)),)) if d.group(3) else (d.group(2), kind))
    return np.dtype(fields)


def parse(text: str) -> Abi:
    abi = Abi()
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group().count("\n"), text, flags=re.S)      # keeps line numbers
    block = _BLOCK.search(text)
    if not block:
        raise AbiError('pygmu_hip.h: no extern "C" block')
    pos, end = block.span(1)
    line, counted = 1, 0
    while True:
        pos = _SPACE.match(text, pos, end).end()
        if pos >= end:
            return abi
        line, counted = line + text.count("\n", counted, pos), pos
        if m := _DEFINE.match(text, pos, end):
            abi.constants[m.group(1)] = _evaluate(m.group(2), abi.constants, line)
        elif m := _ENUM.match(text, pos, end):
            for item in filter(None, (s.strip() for s in m.group(1).split(","))):
                name, _, value = item.partition("=")
                abi.constants[name.strip()] = _evaluate(value, abi.constants, line)
        elif m := _STRUCT.match(text, pos, end):
            abi.structs[m.group(2)] = _dtype(m.group(1), abi.structs, line)
        elif m := _ALIAS.match(text, pos, end):
            if m.group(1) not in abi.structs or m.group(2) in abi.structs or m.group(2) in abi.aliases:
                raise AbiError(f"pygmu_hip.h:{line}: {m.group(2)!r} must be a new name for an earlier struct, "
                               f"which {m.group(1)!r} is not")
            abi.aliases[m.group(2)] = m.group(1)
        elif m := _PROTOTYPE.match(text, pos, end):
            known = abi.structs.keys() | abi.aliases.keys()
            restype, name = _ctype(m.group(1), known, line, returned=True)
            params = [] if m.group(2).strip() == "void" else m.group(2).split(",")
            abi.functions[name] = (restype, [_ctype(p, known, line)[0] for p in params])
        else:
            raise AbiError(f"pygmu_hip.h:{line}: not a #define, enum, struct or prototype: "
                           f"{text[pos:end].splitlines()[0]!r}")
        pos = m.end()


def load(path: str) -> Abi:
    try:
        with open(path) as f:
            text = f.read()
    except OSError as e:
        raise RuntimeError(f"cannot read the ABI header {path}: {e}") from None
    return parse(text)
