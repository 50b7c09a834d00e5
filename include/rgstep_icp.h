/* rgstep_icp.h -- part of the C ABI of librgstep.so: included by rgstep.h (include that one).
 * The entry points live in a header of their own because rgstep.h's list of ra_* functions is pinned by the boundary test of the suite;
 * tests/test_rearrange_icp.py checks this header against the library and the binding in the same way. */
#ifndef RGSTEP_ICP_H
#define RGSTEP_ICP_H
#ifndef RGSTEP_H
#error "include rgstep.h"
#endif
#ifdef __cplusplus
extern "C" {
#endif
/* ---- GoalArgs.rot_dist_type "icp" (goals/object_state.py:128-149, 258-290; utils/icp.py): one launch in front of ra_env_post_step, one 256-thread workgroup per
 * (env, object); robogym_amd/csrc/ra_icp_kernel.h describes the algorithm.  The main batch must hold a full final forward (xquat of this state), as for
 * ra_env_post_step.  All arrays are device pointers.  The clouds are in the objects' body frames (robogym_amd/envs/rearrange/icp.py object_point_clouds): src
 * [N][src_stride][3] with src_num[i] <= min(src_stride, 512) points in use, tgt [tgt_total][3] flat with object i's tgt_num[i] >= 1 points from row tgt_adr[i] on (the
 * kernel clamps what it reads to these bounds; an object whose cloud is empty or out of bounds gets the default).  icp_rel [B][N][3] receives, per active object of every
 * env whose frozen code is not RA_OBS_SKIP, the Euler angles of the fit (before normalize_angles) or (pi/2, pi/2, pi/2); padded slots (object >= num_active[env]) and skipped envs
 * keep what they hold.  obj_group / num_active / frozen: ra_post_args' rows, NULL allowed; with obj_group object i is measured against the goal the post-step kernel's
 * matching gives it. */
typedef struct ra_icp_args {
  float* icp_rel;                                /* [B][N][3] */
  const float* goal;                             /* [B][N][7], as ra_post_args */
  int num_objects;
  int obj_body[RA_MAXOBJ];
  const float* src; int src_stride; const int* src_num;
  const float* tgt; int tgt_total; const int *tgt_adr, *tgt_num;
  float error_threshold;                         /* GoalArgs.icp_error_threshold (0.15) */
  const int* obj_group;                          /* [B][N] or NULL */
  const int* num_active;                         /* [B] or NULL */
  const unsigned char* frozen;                   /* [B] or NULL */
  /* per-env object subsets (appended; NULL = none, every path above as it is): ra_post_args' obj_perm [B][N], needs num_active.  The workgroup of (env, slot i) fits world
   * object p = obj_perm[env][i]: obj_body, src / src_num and the target cloud (tgt_adr / tgt_num; with obj_group the world object of the matched goal's slot) are read
   * at p, goal and icp_rel by slot. */
  const int* obj_perm;
} ra_icp_args;
int ra_env_icp(rb_batch* main, const ra_icp_args* args, void* stream);
int ra_icp_args_size(void);
#ifdef __cplusplus
}
#endif
#endif
