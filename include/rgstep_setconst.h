/* rgstep_setconst.h -- part of the C ABI of librgstep.so: included by rgstep.h (include that one).
 * The entry point lives in a header of its own because rgstep.h's list of rb_* functions is pinned by the boundary test of the suite;
 * tests/test_large_setconst.py checks this header against the library and the binding in the same way. */
#ifndef RGSTEP_SETCONST_H
#define RGSTEP_SETCONST_H
#ifndef RGSTEP_H
#error "include rgstep.h"
#endif
#ifdef __cplusplus
extern "C" {
#endif
/* mj_setConst on the large-model stepper for the envs of `mask_dev` (int [B] device pointer, NULL: all) -- `mujoco_simulation.set_constants()` of the reference's
 * dactyl `_reset` (envs/dactyl/common/cube_env.py:346-349, mujoco/simulation_interface.py:199-201 of the reference), the counterpart of
 * rg_batch_set_constants: recomputes dof_invweight0 / body_invweight0 / tendon_invweight0 in each env's parameter block (rb_prm_layout) from that block's body_pos /
 * body_mass / body_inertia / dof_armature / site_pos / geom_pos at qpos0 (rb_setconst_kernel: one workgroup per env on the model's kernel configuration).  A masked
 * env's block is left as it is.  stat_meaninertia, body_subtreemass, actuator_acc0 and tendon_length0 stay the model's.  The frame arrays of a recomputed env's scratch
 * row hold the qpos0 configuration afterwards (the next step launch rebuilds them).  A failed factorisation sets RG_STATUS_BAD_FACTOR in the env's status word.
 * Asynchronous on `stream`; fails with a message on a model without rb_model_enable_env_params, and, being not recordable, between rb_multi_begin and rb_multi_launch. */
int rb_batch_set_constants(rb_batch* b, const int* mask_dev /* may be NULL: all */, void* stream);
#ifdef __cplusplus
}
#endif
#endif
