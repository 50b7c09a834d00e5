"""The declarations of a C header as ctypes: structs, integer constants and function prototypes (what robogym_amd/_native.py binds librgstep.so with).

It reads the subset of C that include/rgstep.h is written in and refuses everything else with a NativeError that names the declaration: a field or a parameter
that is skipped silently would shift every member behind it.  Understood: comments, include guards, `#ifdef __cplusplus` blocks (dropped), `#include "file"`
(followed), `#define NAME <integer expression>`, anonymous enums, `typedef struct T T;` (an opaque handle), `typedef struct T { ... } T;` with scalar, pointer,
array and nested-struct members, and prototypes.  Not understood, hence refused: bit-fields, function pointers, unions, unknown type names, function-like
macros, `#if` expressions, array bounds that are no integer expression of known constants.
"""
import ast
import ctypes
import operator
import os
import re


class NativeError(RuntimeError):
    pass


_SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float, "size_t": ctypes.c_size_t, "long long": ctypes.c_longlong,
            "unsigned long long": ctypes.c_ulonglong, "unsigned char": ctypes.c_ubyte, "char": ctypes.c_char, "void": None}
_OPAQUE = object()      # the base type of a handle: usable behind a pointer only
_BINARY = {ast.Add: operator.add, ast.Sub: operator.sub, ast.Mult: operator.mul, ast.LShift: operator.lshift, ast.RShift: operator.rshift,
           ast.BitOr: operator.or_, ast.BitAnd: operator.and_}
_UNARY = {ast.USub: operator.neg, ast.Invert: operator.invert}


class Header:
    """constants: name -> int.  structs: C name -> ctypes.Structure class.  functions: name -> (header file, restype, argtypes).  All in declaration order."""

    def __init__(self):
        self.constants, self.structs, self.functions = {}, {}, {}
        self._opaque, self._defined = set(), set()      # handles declared without a body; every `#define`d name (what `#ifndef` asks about)

    def exports(self, header):
        """The functions a header file declares itself (not the files it includes)."""
        return [name for name, (h, _, _) in self.functions.items() if h == header]

    def parse_file(self, path):
        with open(path) as f:
            self.parse(f.read(), os.path.basename(path), os.path.dirname(path))

    def parse(self, text, header="<string>", include_dir=None):
        for stmt in self._statements(text, header):
            if m := re.match(r"__define (\w+) (.+)$", stmt):
                self._constant(m.group(1), self._int(m.group(2), stmt))
            elif m := re.match(r"__include (\S+)$", stmt):
                if include_dir is None:
                    raise NativeError("%s: no directory to find `%s` in" % (header, m.group(1)))
                self.parse_file(os.path.join(include_dir, m.group(1)))
            elif m := re.match(r"typedef struct (\w+) (\1)$", stmt):
                self._opaque.add(m.group(1))
            elif m := re.match(r"enum \{(.*)\}$", stmt):
                value = -1
                for member in filter(None, (s.strip() for s in m.group(1).split(","))):
                    name, eq, expr = (s.strip() for s in member.partition("="))
                    value = self._int(expr, stmt) if eq else value + 1
                    self._constant(name, value)
            elif m := re.match(r"typedef struct (\w+) \{([^{}]*)\} (\1)$", stmt):
                name = m.group(1)
                if name in self.structs:
                    raise NativeError("%s: struct %s is defined twice" % (header, name))
                fields = [f for decl in m.group(2).split(";") if decl.strip() for f in self._members(decl.strip(), name)]
                self.structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields, "__doc__": "`%s` of include/%s, as the header declares it." % (name, header)})
            elif m := re.match(r"([^{}()]*?)\b(\w+) ?\(([^{}()]*)\)$", stmt):
                ret, name, params = m.groups()
                if name in self.functions:
                    raise NativeError("%s: %s is declared twice" % (header, name))
                params = [] if params.strip() in ("", "void") else [self._parameter(p.strip(), stmt) for p in params.split(",")]
                self.functions[name] = (header, self._parameter(ret.strip(), stmt, returns=True), params)
            else:       # a union, a named enum, a nested aggregate, a function pointer, a variable ...
                raise NativeError("%s: not understood: %s" % (header, stmt))

    # ---- text -> statements

    def _statements(self, text, header):
        """Comments out, preprocessor lines handled (a `#define` with a body and an `#include "file"` become statements of their own), the rest split at the `;`
        outside braces; whitespace collapsed."""
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
        lines, skipping = [], []          # skipping: one entry per open conditional, True where C would not read the block
        for line in text.split("\n"):
            s = line.strip()
            if not s.startswith("#"):
                if not any(skipping):
                    lines.append(line)
                continue
            word, _, rest = s[1:].strip().partition(" ")
            rest = rest.strip()
            if word == "ifndef" and re.match(r"\w+$", rest):
                skipping.append(rest in self._defined)
            elif (word, rest) == ("ifdef", "__cplusplus"):
                skipping.append(True)
            elif word == "endif" and skipping:
                skipping.pop()
            elif any(skipping):
                continue
            elif word == "define" and re.match(r"\w+$", rest):          # an include guard
                self._defined.add(rest)
            elif word == "define" and re.match(r"\w+\s", rest) and not s.endswith("\\"):
                self._defined.add(rest.split()[0])
                lines.append("__define %s;" % rest)
            elif word == "include" and re.match(r'"[^"]+"$', rest):
                lines.append("__include %s;" % rest[1:-1])
            elif not (word == "include" and re.match(r"<[^>]+>$", rest)):
                raise NativeError("%s: preprocessor line not understood: %s" % (header, s))
        if skipping:
            raise NativeError("%s: unterminated #if" % header)
        out, depth, start, text = [], 0, 0, "\n".join(lines)
        for i, ch in enumerate(text):
            depth += (ch == "{") - (ch == "}")
            if ch == ";" and depth == 0:
                out.append(" ".join(text[start:i].split()))
                start = i + 1
        if depth != 0 or text[start:].strip():
            raise NativeError("%s: not understood: %s" % (header, " ".join(text[start:].split())[:120]))
        return [s for s in out if s]

    # ---- constants

    def _constant(self, name, value):
        if not re.match(r"[A-Za-z_]\w*$", name) or self.constants.get(name, value) != value:
            raise NativeError("constant %s: not a name, or defined twice with different values" % name)
        self.constants[name] = value

    def _int(self, expr, where):
        """An integer constant expression of C: literals (with u / l suffixes), known constants, + - * << >> | & ~ and parentheses."""
        def ev(node):
            if isinstance(node, ast.Constant) and type(node.value) is int:
                return node.value
            if isinstance(node, ast.Name) and node.id in self.constants:
                return self.constants[node.id]
            if isinstance(node, ast.BinOp) and type(node.op) in _BINARY:
                return _BINARY[type(node.op)](ev(node.left), ev(node.right))
            if isinstance(node, ast.UnaryOp) and type(node.op) in _UNARY:
                return _UNARY[type(node.op)](ev(node.operand))
            raise NativeError("no integer constant expression: `%s` in: %s" % (expr, where))
        try:
            return ev(ast.parse(re.sub(r"\b(0[xX][0-9a-fA-F]+|\d+)[uUlL]+\b", r"\1", expr.strip()), mode="eval").body)
        except SyntaxError:
            raise NativeError("no integer constant expression: `%s` in: %s" % (expr, where)) from None

    # ---- types

    def _base(self, words, where):
        """The longest leading run of `words` (identifiers, `const` dropped) that names a type -> (type, the words left over)."""
        words = [w for w in words if w != "const"]
        for n in range(len(words), 0, -1):
            name = " ".join(words[:n])
            if name in _SCALARS:
                return _SCALARS[name], words[n:]
            if n == 1 and name in self.structs:
                return self.structs[name], words[1:]
            if n == 1 and name in self._opaque:
                return _OPAQUE, words[1:]
        raise NativeError("unknown type `%s` in: %s" % (" ".join(words), where))

    @staticmethod
    def _ctype(base, stars, where):
        if stars == 0:
            if base is _OPAQUE:
                raise NativeError("an opaque struct by value in: %s" % where)
            return base
        if stars == 1 and base is ctypes.c_char:
            return ctypes.c_char_p
        if stars == 1 and isinstance(base, type) and issubclass(base, ctypes.Structure):
            return ctypes.POINTER(base)
        return ctypes.c_void_p

    def _declaration(self, decl, where):
        """`const float *lo, *hi`, `float half[RA_MAXOBJ][3]`, `unsigned` or `const char*` -> [(name or "", ctype or None for void), ...], one per declarator."""
        m = re.match(r"((?:[A-Za-z_]\w*\s+)*[A-Za-z_]\w*)\s*([^():]*)$", decl)
        if not m:
            raise NativeError("not understood (a bit-field, a function pointer?): `%s` in: %s" % (decl, where))
        base, left = self._base(m.group(1).split(), where)      # left: the first declarator's name, when no `*` stands before it
        if len(left) > 1 or (left and m.group(2).startswith("*")):
            raise NativeError("unknown type in `%s` in: %s" % (decl, where))
        out = []
        for d in ("".join(left) + m.group(2)).split(","):
            m = re.match(r"\s*(\**)\s*((?:[A-Za-z_]\w*)?)\s*((?:\[[^\]]*\]\s*)*)$", d)
            if not m:
                raise NativeError("not understood: `%s` of `%s` in: %s" % (d.strip(), decl, where))
            ctype = self._ctype(base, len(m.group(1)), where)
            for bound in reversed(re.findall(r"\[([^\]]*)\]", m.group(3))):
                n = self._int(bound, where) if bound.strip() else 0
                if n <= 0 or ctype is None:
                    raise NativeError("array `%s` in: %s" % (d.strip(), where))
                ctype = ctype * n
            out.append((m.group(2), ctype))
        return out

    def _members(self, decl, struct):
        """One member declaration of a struct -> [(name, ctype), ...]: every declarator has a name and a size."""
        where = "%s { %s; }" % (struct, decl)
        fields = self._declaration(decl, where)
        if any(not name or ctype is None for name, ctype in fields):
            raise NativeError("a member without a name or of type void: %s" % where)
        return fields

    def _parameter(self, text, where, returns=False):
        """A parameter (`const int* mask_dev`, `unsigned`) or, with `returns`, a return type -> ctype (None: void, a return type only)."""
        (name, ctype), = self._declaration(text, where)         # (the caller split at the commas: one declarator)
        is_array = isinstance(ctype, type) and issubclass(ctype, ctypes.Array)
        if is_array or (returns and name) or (ctype is None and not (returns and text == "void")):
            raise NativeError("not understood: `%s` in: %s" % (text, where))
        return ctype
