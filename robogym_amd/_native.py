"""ctypes binding of librgstep.so (the gfx950 HIP stepper behind the C ABI of include/rgstep.h).

The binding is generated from the header when this module is imported (robogym_amd/_cabi.py reads include/rgstep.h and the headers it includes): the argument
structs, every integer `#define` and enum member, and the return and parameter types of every function.  The header is the one place a struct's layout is
written down.  bind() still compares each `*_args_size()` of the loaded library with the parsed struct: that tells a library built from another version of the
header (a stale librgstep.so) from the header next to this package.

There is no CPU fallback: if the library is missing or no MI355X is visible the product raises.
"""
import ctypes
import os

from ._cabi import Header, NativeError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RGSTEP_LIB") or os.path.join(_HERE, "csrc", "librgstep.so")   # (RGSTEP_LIB: A/B builds of the same ABI, tools/ only)

ABI = Header()
ABI.parse_file(os.path.join(_HERE, "..", "include", "rgstep.h"))      # (where robogym_amd/csrc/Makefile finds it)
globals().update(ABI.constants)      # RG_F_*, RB_F_*, RG_STATUS_*, RG_FLAG_*, RG_CFG_*, RG_WK_*, RA_*, *_NDRAW, ...: the header's names and values

StepArgs, PostArgs = ABI.structs["rg_step_args"], ABI.structs["rg_post_args"]
WrapDims, WrapLay, WrapArgs = ABI.structs["rg_wrap_dims"], ABI.structs["rg_wrap_lay"], ABI.structs["rg_wrap_args"]
RbPostArgs, RbTcpArgs = ABI.structs["rb_post_args"], ABI.structs["rb_tcp_args"]
RaPostArgs, RaIcpArgs, RaRecipeArgs, RaParamRowsArgs = (ABI.structs[n] for n in ("ra_post_args", "ra_icp_args", "ra_recipe_args", "ra_param_rows_args"))

# the functions each header file declares (tests pin rgstep.h's own list, so later entry points live in headers that it includes)
EXPORTS, EXPORTS_SETCONST = ABI.exports("rgstep.h"), ABI.exports("rgstep_setconst.h")
EXPORTS_ICP, EXPORTS_SYNC_RESET = ABI.exports("rgstep_icp.h"), ABI.exports("rgstep_sync_reset.h")

# What the header does not carry.  The packed row's keys in RG_WK_* order, under the reference's names (the enum abbreviates them; "_delta": the block of the
# RandomizedBodyWrapper family's entries):
RG_WRAP_KEYS = ["cube_pos", "cube_quat", "qpos", "qvel", "hand_angle", "fingertip_pos", "goal_pos", "goal_quat", "qpos_goal", "is_goal_achieved", "fell_down", "action_history",
                "action_delay", "_delta", "noisy_cube_pos", "noisy_cube_quat", "noisy_fingertip_pos", "noisy_hand_angle", "action_ema", "achieved_goal_pos", "relative_goal_pos",
                "noisy_achieved_goal_pos", "noisy_relative_goal_pos", "achieved_goal_quat", "relative_goal_quat", "noisy_achieved_goal_quat", "noisy_relative_goal_quat",
                "relative_goal", "noisy_relative_goal", "achieved_goal", "noisy_achieved_goal", "goal", "previous_action", "reward"]
assert len(RG_WRAP_KEYS) == ABI.constants["RG_WK_COUNT"], "RG_WRAP_KEYS and the RG_WK_* enum of include/rgstep.h disagree"
# The per-env parameter fields in the order of the internal rb_types.h (RB_P_*) / rg_types.h: their lengths are checked against rb_prm_layout / rg_prm_layout of
# the loaded library where they are used (LargeEnvParams, prm_layout below).
RB_PRM_NAMES = ["gravity", "dof_damping", "dof_armature", "dof_frictionloss", "dof_invweight0", "jnt_stiffness", "jnt_margin", "jnt_range", "body_pos", "body_mass", "body_inertia",
                "body_invweight0", "actuator_gainprm", "actuator_forcerange", "actuator_ctrlrange", "geom_pos", "geom_margin", "geom_gap", "geom_friction", "geom_solref", "geom_solimp",
                "tendon_range", "tendon_invweight0", "timestep", "xfrc_applied", "site_pos", "geom_scale"]
PRM_NAMES = ["row", "gravity", "timestep", "dof_damping", "dof_armature", "dof_frictionloss", "dof_invweight0", "body_mass", "body_inertia", "body_invweight0",
             "jnt_range", "tendon_range", "tendon_invweight0", "actuator_gainprm", "actuator_ctrlrange", "actuator_forcerange", "geom_friction", "xfrc_applied", "site_pos", "geom_scale", "jnt_margin", "geom_solref", "geom_solimp"]


def bind(path):
    """Load a build of the C ABI and declare the signature of every function the header declares."""
    if not os.path.exists(path):
        raise NativeError(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % path
        )
    L = ctypes.CDLL(path)
    for name, (header, restype, argtypes) in ABI.functions.items():
        if not hasattr(L, name):
            raise NativeError("%s does not export %s, which include/%s declares" % (path, name, header))
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    for name, struct in ABI.structs.items():
        if name + "_size" in ABI.functions and getattr(L, name + "_size")() != ctypes.sizeof(struct):
            raise NativeError("%s layout mismatch: %s was built from another version of the header than the include/ next to robogym_amd" % (name, path))
    return L


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        _LIB = bind(LIB_PATH)
    return _LIB


def check(L, rc, what):
    if rc != 0:
        raise NativeError("%s failed: %s" % (what, L.rg_last_error().decode()))


def prm_layout(L):
    """rg_prm_layout as a dict: 'row' -> floats per env, then field -> offset."""
    buf = (ctypes.c_int * 32)()
    n = L.rg_prm_layout(buf, 32)
    assert n == len(PRM_NAMES), "rg_prm_layout and robogym_amd/_native.py disagree"
    return {k: int(buf[i]) for i, k in enumerate(PRM_NAMES)}
