"""The binding that robogym_amd/_native.py generates from include/rgstep.h against the hand-written one of an earlier commit: struct layouts, integer
constants and the signature of every function, side by side.  The earlier _native.py is taken out of git and loaded as a module next to the current one; both
bind the same library (any build of the ABI; default: the emulator build).

    python tools/abi_identity.py [REV, default HEAD^] [library]       exit status 1 on a difference that is more than a pointer's class
"""
import ctypes
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robogym_amd import _native as new      # noqa: E402

STRUCTS = {"StepArgs": "rg_step_args", "PostArgs": "rg_post_args", "WrapDims": "rg_wrap_dims", "WrapLay": "rg_wrap_lay", "WrapArgs": "rg_wrap_args", "RbTcpArgs": "rb_tcp_args",
           "RbPostArgs": "rb_post_args", "RaPostArgs": "ra_post_args", "RaIcpArgs": "ra_icp_args", "RaRecipeArgs": "ra_recipe_args", "RaParamRowsArgs": "ra_param_rows_args"}


def layout(cls):
    return [(name, getattr(cls, name).offset, getattr(cls, name).size) for name, *_ in cls._fields_]


def type_name(t, struct_names):
    if t is None:
        return "void"
    if hasattr(t, "_type_") and not isinstance(t._type_, str):      # POINTER(x)
        return "POINTER(%s)" % struct_names.get(t._type_, t._type_.__name__)
    return t.__name__


def main():
    rev = sys.argv[1] if len(sys.argv) > 1 else "HEAD^"
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "emul", "librgstep_emul.so")
    old = types.ModuleType("parent_native")
    old.__file__ = os.path.join(ROOT, "robogym_amd", "_native.py")
    exec(compile(subprocess.check_output(["git", "-C", ROOT, "show", rev + ":robogym_amd/_native.py"]).decode(), "parent _native.py", "exec"), old.__dict__)
    bad = 0

    print("== structs: (field, offset, size) lists and sizeof, parent | generated")
    for py, c in STRUCTS.items():
        a, b = getattr(old, py), getattr(new, py)
        same = layout(a) == layout(b) and ctypes.sizeof(a) == ctypes.sizeof(b) and b is new.ABI.structs[c]
        bad += not same
        print("%-18s %-20s fields %3d | %3d   sizeof %5d | %5d   %s" % (py, c, len(a._fields_), len(b._fields_), ctypes.sizeof(a), ctypes.sizeof(b), "equal" if same else "DIFFERENT"))
        for fa, fb in zip(layout(a), layout(b)):
            print("    %-32s %5d %4d | %-32s %5d %4d%s" % (fa + fb + ("" if fa == fb else "   DIFFERENT",)))

    print("== integer constants of the parent binding in the generated one")
    consts = {k: v for k, v in vars(old).items() if k.isupper() and type(v) is int}
    wrong = {k: (v, getattr(new, k, None)) for k, v in consts.items() if getattr(new, k, None) != v or type(getattr(new, k)) is not int}
    bad += len(wrong)
    print("%d constants, %d missing or different %s" % (len(consts), len(wrong), wrong or ""))
    print("generated only: %s" % " ".join(sorted(k for k in new.ABI.constants if k not in consts)))
    for k in ("EXPORTS", "EXPORTS_SETCONST", "EXPORTS_ICP", "EXPORTS_SYNC_RESET"):
        same = set(getattr(old, k)) == set(getattr(new, k)) and len(getattr(old, k)) == len(getattr(new, k))
        bad += not same
        print("%-20s %2d | %2d names   %s" % (k, len(getattr(old, k)), len(getattr(new, k)), "equal sets" if same else "DIFFERENT"))

    print("== functions: restype (argtypes), parent | generated.  `-` = the parent left it undeclared (ctypes then converts each argument by its Python type)")
    La, Lb = old.bind(path), new.bind(path)
    names = {a: c for c, a in ((c, getattr(old, py)) for py, c in STRUCTS.items())}
    names.update({new.ABI.structs[c]: c for c in STRUCTS.values()})
    pointers = ("c_void_p", "c_char_p", "POINTER(")
    listed = []
    for fn in old.EXPORTS + old.EXPORTS_SETCONST + old.EXPORTS_ICP + old.EXPORTS_SYNC_RESET:
        fa, fb = getattr(La, fn), getattr(Lb, fn)
        ra, rb = type_name(fa.restype, names), type_name(fb.restype, names)
        aa = None if fa.argtypes is None else [type_name(t, names) for t in fa.argtypes]
        ab = [type_name(t, names) for t in fb.argtypes]
        if (ra, aa) == (rb, ab):
            verdict = "equal"
        elif (ra, rb) == ("c_int", "void") and aa == ab and fa.restype is ctypes.c_int:
            verdict = "void in the header: the parent left ctypes' default int restype (a value no caller reads)"
        elif ra == rb and aa is None:
            verdict = "parent undeclared" if ab else "equal (no parameters; parent undeclared)"
        elif ra == rb and len(aa) == len(ab) and all(x == y or (x.startswith(pointers) and y.startswith(pointers)) for x, y in zip(aa, ab)):
            verdict = "pointer class: " + ", ".join("#%d %s -> %s" % (i, x, y) for i, (x, y) in enumerate(zip(aa, ab)) if x != y)
        else:
            verdict, bad = "DIFFERENT", bad + 1
        if not verdict.startswith("equal"):
            listed.append(fn)
        print("%-28s %s (%s) | %s (%s)   %s" % (fn, ra, "-" if aa is None else ", ".join(aa), rb, ", ".join(ab), verdict))
    print("%d functions; %d differ in a pointer's class, return void or were undeclared in the parent: %s" %(len(new.ABI.functions), len(listed), " ".join(listed)))
    print("RESULT: %s" % ("DIFFERENT (%d)" % bad if bad else "identical layouts, constants and signatures up to the pointer classes listed"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
