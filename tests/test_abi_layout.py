"""The binding is generated from include/rgstep.h (robogym_amd/_cabi.py): what the parser reads out of the header against what the C compiler makes of the same
header -- every field's offset and size, every struct's size, every integer constant's value --, every prototype bound on the emulator build of the ABI, and the
parser's refusals."""
import ctypes
import os
import re
import subprocess

import pytest

from robogym_amd import _cabi, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADERS = ("rgstep.h", "rgstep_setconst.h", "rgstep_icp.h", "rgstep_sync_reset.h")


def _header_text():
    """The four headers without their comments (the tests below find names in it with regular expressions of their own, not with the parser)."""
    return "\n".join(re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(os.path.join(INCLUDE, h)).read(), flags=re.S) for h in HEADERS)


def _constant_names(text):
    names = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+\S", text, flags=re.M)
    for body in re.findall(r"\benum\s*\{([^}]*)\}", text):
        names += [member.split("=")[0].strip() for member in body.split(",") if member.strip()]
    return names


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """A C program that includes rgstep.h and prints offsetof / sizeof of every parsed field, sizeof of every struct and the value of every constant the
    regular expressions above find; compiled as C with the host compiler, run once.  -> {"S": size, "S.f": (offset, size), "NAME": value}"""
    d = tmp_path_factory.mktemp("abi")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rgstep.h"', 'int main(void) {']
    for name, cls in _native.ABI.structs.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        for field, *_ in cls._fields_:
            lines.append('  printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (name, field, name, field, name, field))
    for name in _constant_names(_header_text()):
        lines.append('  printf("%s %%lld\\n", (long long)(%s));' % (name, name))
    lines += ['  return 0;', '}']
    src, exe = d / "abi_layout.c", d / "abi_layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)])      # (also: the header is valid C)
    out = {}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        key, *values = line.split()
        out[key] = tuple(int(v) for v in values) if len(values) > 1 else int(values[0])
    return out


def test_every_struct_matches_the_c_compiler(compiled):
    assert len(_native.ABI.structs) == 11
    for name, cls in _native.ABI.structs.items():
        assert ctypes.sizeof(cls) == compiled[name], name
        for field, *_ in cls._fields_:
            desc = getattr(cls, field)
            assert (desc.offset, desc.size) == compiled["%s.%s" % (name, field)], "%s.%s" % (name, field)
    # the public aliases are these classes
    for alias, name in (("StepArgs", "rg_step_args"), ("PostArgs", "rg_post_args"), ("WrapDims", "rg_wrap_dims"), ("WrapLay", "rg_wrap_lay"), ("WrapArgs", "rg_wrap_args"),
                        ("RbTcpArgs", "rb_tcp_args"), ("RbPostArgs", "rb_post_args"), ("RaPostArgs", "ra_post_args"), ("RaIcpArgs", "ra_icp_args"),
                        ("RaRecipeArgs", "ra_recipe_args"), ("RaParamRowsArgs", "ra_param_rows_args")):
        assert getattr(_native, alias) is _native.ABI.structs[name]


def test_no_member_of_a_struct_is_skipped():
    """The number of fields per struct, counted without the parser: a member declaration contributes one field per comma-separated declarator."""
    text = _header_text()
    for name, cls in _native.ABI.structs.items():
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
        assert len(cls._fields_) == sum(decl.count(",") + 1 for decl in body.split(";") if decl.strip()), name


def test_every_constant_is_an_attribute_with_the_compilers_value(compiled):
    names = _constant_names(_header_text())
    assert len(names) > 90 and len(set(names)) == len(names) and set(names) == set(_native.ABI.constants)
    for name in names:
        assert type(getattr(_native, name)) is int and getattr(_native, name) == compiled[name], name
    assert _native.RG_POST_NDRAW == 29 and _native.RG_STATUS_SCHED == 64 and _native.RG_WK_COUNT == len(_native.RG_WRAP_KEYS)     # an expression, a `u` suffix, an enum's last member
    assert _native.RG_FLAG_SENSORS == 32


def test_every_prototype_is_bound_on_the_emulator_library(emul_lib):
    text = _header_text()
    protos = dict(re.findall(r"\b(r[gba]_\w+)\s*\(([^()]*)\)\s*;", text))
    assert len(protos) == 71 and set(protos) == set(_native.ABI.functions)
    assert set(protos) == set(_native.EXPORTS + _native.EXPORTS_SETCONST + _native.EXPORTS_ICP + _native.EXPORTS_SYNC_RESET)
    for name, params in protos.items():
        fn = getattr(emul_lib, name)
        assert len(fn.argtypes) == (0 if params.strip() in ("", "void") else params.count(",") + 1), name
        header, restype, argtypes = _native.ABI.functions[name]
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert emul_lib.rg_blob_free.restype is None and emul_lib.rg_last_error.restype is ctypes.c_char_p and emul_lib.rg_batch_field_ptr.restype is ctypes.c_void_p
    assert emul_lib.rg_batch_step_ex.argtypes == [ctypes.c_void_p, ctypes.POINTER(_native.StepArgs)]
    assert emul_lib.rg_model_create.argtypes == [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_int]


def test_a_library_without_a_declared_function_is_refused(tmp_path):
    (tmp_path / "partial.c").write_text("int rg_blob_entry(void) { return 0; }\n")      # the header's first function, and nothing else
    subprocess.check_call(["cc", "-shared", "-fPIC", "-o", str(tmp_path / "partial.so"), str(tmp_path / "partial.c")])
    with pytest.raises(_native.NativeError, match="does not export rg_compile_mjcf, which include/rgstep.h declares"):
        _native.bind(str(tmp_path / "partial.so"))


SYNTHETIC = {
    "bit-field": "typedef struct s { int a : 3; int b; } s;",
    "function pointer member": "typedef struct s { int a; void (*done)(int); } s;",
    "function pointer parameter": "int f(int (*callback)(int));",
    "unknown type": "typedef struct s { int a; uint64_t b; } s;",
    "unknown parameter type": "int f(rg_unknown* p);",
    "union": "typedef union u { int a; float b; } u;",
    "union member": "typedef struct s { union { int a; float b; } v; } s;",
    "array bound": "typedef struct s { int a[N_UNKNOWN]; } s;",
    "empty array bound": "typedef struct s { int n; int a[]; } s;",
    "opaque by value": "typedef struct h h;\ntypedef struct s { h handle; } s;",
    "void member": "typedef struct s { void a; } s;",
    "function-like macro": "#define TWICE(x) (2 * (x))",
    "float constant": "#define HALF 0.5",
    "conditional": "#if 1\n#define A 1\n#endif",
    "continued line": "#define A 1 + \\\n 2",
    "variable": "extern int rg_count;",
    "unterminated": "typedef struct s { int a; } s",
}


@pytest.mark.parametrize("what", sorted(SYNTHETIC))
def test_the_parser_refuses_what_it_does_not_understand(what):
    h = _cabi.Header()
    with pytest.raises(_native.NativeError):
        h.parse(SYNTHETIC[what])
    assert not h.structs and not h.functions


def test_a_side_header_on_its_own_is_refused_as_the_compiler_refuses_it():
    with pytest.raises(_native.NativeError, match='#error "include rgstep.h"'):
        _cabi.Header().parse_file(os.path.join(INCLUDE, "rgstep_icp.h"))


def test_the_parser_reads_the_subset_the_header_is_written_in():
    h = _cabi.Header()
    h.parse("""#ifndef G_H
#define G_H
#ifdef __cplusplus
extern "C" {
#endif
/* a comment with a ; and a { in it */
#define N (2 + 4 + 3 + 20)   // and one of these
#define BIT 64u
enum { A, B = 5, C, D = N | BIT };
typedef struct h h;
typedef struct in { int x, y; } in;
typedef struct s {
  const float *lo, *hi; int n;
  unsigned char flag; unsigned seed, step;
  float m[C][2];       /* C == 6 */
  in inner; unsigned long long mask; const char* name; long long big; size_t bytes;
} s;
h* make(const void* blob, size_t nbytes, char* err, int errlen);
void drop(h* handle);
int run(const h* handle, const s* args /* may be NULL */, void** out, unsigned, float scale);
const char* last_error(void);
#ifdef __cplusplus
}
#endif
#endif
""")
    assert h.constants == {"N": 29, "BIT": 64, "A": 0, "B": 5, "C": 6, "D": 29 | 64}
    S, In = h.structs["s"], h.structs["in"]
    assert [(n, t) for n, t in S._fields_] == [("lo", ctypes.c_void_p), ("hi", ctypes.c_void_p), ("n", ctypes.c_int), ("flag", ctypes.c_ubyte), ("seed", ctypes.c_uint),
                                               ("step", ctypes.c_uint), ("m", (ctypes.c_float * 2) * 6), ("inner", In), ("mask", ctypes.c_ulonglong),
                                               ("name", ctypes.c_char_p), ("big", ctypes.c_longlong), ("bytes", ctypes.c_size_t)]
    assert h.functions == {"make": ("<string>", ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_int]),
                           "drop": ("<string>", None, [ctypes.c_void_p]),
                           "run": ("<string>", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(S), ctypes.c_void_p, ctypes.c_uint, ctypes.c_float]),
                           "last_error": ("<string>", ctypes.c_char_p, [])}
    assert h.exports("<string>") == ["make", "drop", "run", "last_error"]
