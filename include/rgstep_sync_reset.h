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
 * its six dofs.  A caller whose randomizers change mass or gravity at `episode_started` runs the park stage once more after them.
 * Stage RA_ROWS_MATERIAL (mat_table given; between the two): per-object materials, the reference's `material_names`.  Where `ended` is set every slot takes a
 * material -- obj_material_next[env][slot] where that names a row of the table, else mat_choice[floor(u x num_choice)] with u of a draw stream of its own over
 * (mat_seed, mat_step, env, slot); with obj_group the slots of one group take the material of the group's lowest slot -- which is written to obj_material and
 * applied to the slot's world object: a table row is RA_MAT_WORDS floats, word 0 the RA_MAT_* bits (as a float) that say which of the others are written, a row
 * of zeros (the compiled world's own material) writes nothing.  RA_MAT_MASS: body_mass and body_inertia = block_default's x word 1; RA_MAT_FRICTION / _SOLREF /
 * _SOLIMP: words 2-4 / 5-6 / 7-9 into the rows of the object's geoms (solimp: its first three words); RA_MAT_JOINT: word 11 into the six dofs' armature, and
 * word 10 is the damping that the restore stage gives the object where `stabilised` is set, read through obj_material (a row without the bit: block_default's).
 * With RA_MAT_MASS or RA_MAT_JOINT both _invweight0 rows of the object follow in closed form (a free body that is a tree of its own: obj_lever2; exact where the
 * armature or the lever is zero). */
#define RA_ROWS_RESTORE 1
#define RA_ROWS_PARK 2
#define RA_ROWS_MATERIAL 4
#define RA_MAT_WORDS 12
#define RA_MAT_MASS 1
#define RA_MAT_FRICTION 2
#define RA_MAT_SOLREF 4
#define RA_MAT_SOLIMP 8
#define RA_MAT_JOINT 16
#define RA_MAT_MAXCHOICE 16
#define RA_MAT_NOFF 8
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
  int stages;                                    /* RA_ROWS_RESTORE | RA_ROWS_MATERIAL | RA_ROWS_PARK */
  /* per-object materials (zero / NULL = none, every path above as it is).  These members stand in front of obj_perm, which stays the struct's last member; a caller
   * built against another version of this header is told by the size the library reports. */
  const float* mat_table;                        /* [num_materials][RA_MAT_WORDS] */
  int num_materials;
  int num_choice;                                /* 1..RA_MAT_MAXCHOICE */
  int mat_choice[RA_MAT_MAXCHOICE];              /* rows of mat_table a draw picks from, with multiplicity */
  int* obj_material;                             /* [B][N] the material of every slot; written where `ended` is set */
  const int* obj_material_next;                  /* [B][N] the pin: a row of mat_table, or -1 (anything outside the table) = drawn.  Read at every episode start, never cleared */
  unsigned mat_seed, mat_step;
  const int* obj_group;                          /* [B][N] or NULL: ra_recipe_args' row as the recipe launch left it */
  int obj_geomadr[RA_MAXOBJ], obj_geomnum[RA_MAXOBJ];   /* the geoms of each object's body */
  float obj_lever2[RA_MAXOBJ][3];                /* |body_ipos x principal axis k|^2: what the centre of mass's offset from the free joint adds to the translational dof_invweight0 */
  int mat_off[RA_MAT_NOFF];                      /* word offsets in the scratch row (rb_prm_layout): geom_friction, geom_solref, geom_solimp, body_mass, body_inertia, dof_armature, dof_invweight0, body_invweight0 */
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
