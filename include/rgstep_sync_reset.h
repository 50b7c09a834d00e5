/* rgstep_sync_reset.h -- part of the C ABI of librgstep.so: included by rgstep.h (include that one).
 * The entry points live in a header of their own because rgstep.h's list of ra_* functions is pinned by the boundary test of the suite;
 * tests/test_rearrange_sync_reset.py checks this header against the library and the binding in the same way. */
#ifndef RGSTEP_SYNC_RESET_H
#define RGSTEP_SYNC_RESET_H
#ifndef RGSTEP_H
#error "include rgstep.h"
#endif
#ifdef __cplusplus
extern "C" {
#endif
/* ---- the per-env parameter rows after a launch of the recipe kernel (ra_recipe_args of rgstep.h), on the rows of its masks only: one wave per env, an env outside
 * `active` or with none of its three mask bytes set is skipped.  The main batch must have per-env parameter rows (rb_model_enable_env_params).  All arrays are
 * device pointers.  Stage RA_ROWS_RESTORE: where `ended` is set the whole parameter block becomes block_default (the model's values in the block's layout, what the
 * block held when the batch was made: a re-created simulation, xfrc_applied zero among it); then the six dofs of every object's free joint get stabilize_damping
 * where `ended` is set and block_default's damping where `stabilised` is set (stabilize_objects, common/utils.py:76-92).  Stage RA_ROWS_PARK (num_active given):
 * where any of the three masks is set, every object i >= num_active[env] gets xfrc_applied force = - body_mass x gravity from THAT env's rows and park_damping on
 * its six dofs.  A caller whose randomizers change mass or gravity at `episode_started` runs the park stage once more after them. */
#define RA_ROWS_RESTORE 1
#define RA_ROWS_PARK 2
typedef struct ra_param_rows_args {
  const unsigned char *ended, *stabilised, *episode_started;   /* [B]: ra_recipe_args' masks */
  const unsigned char* active;                   /* [B] or NULL = all envs */
  const float* block_default;                    /* [words of a parameter block] (rb_prm_layout) */
  int num_objects;
  int obj_dofadr[RA_MAXOBJ];                     /* first of the six dofs of each object's free joint */
  int obj_body[RA_MAXOBJ];
  float stabilize_damping;
  const int* num_active;                         /* [B] or NULL: no parking */
  float park_damping;
  int stages;                                    /* RA_ROWS_RESTORE | RA_ROWS_PARK */
  /* per-env object subsets (appended; NULL = none, every path above as it is): ra_recipe_args' obj_perm [B][N] as the recipe launch left it, needs num_active.  The park
   * stage then parks the WORLD objects of the slots >= num_active[env]: obj_body and obj_dofadr are read at obj_perm[env][slot]. */
  const int* obj_perm;
} ra_param_rows_args;
int ra_env_param_rows(rb_batch* main, const ra_param_rows_args* args, void* stream);
int ra_param_rows_args_size(void);
#ifdef __cplusplus
}
#endif
#endif
