// ra_row.h — the packed observation row of the rearrange envs (ra_post_args.obs, include/rgstep.h), described once: the keys in the row's order (OBS_KEYS, then
// MASK_OBS_KEYS of robogym_amd/envs/rearrange/blocks.py) and each key's width.  Offsets and the row's width are sums over this table, folded at compile time; no
// other file does arithmetic on the layout.
#pragma once
namespace rgb {
enum RaKey {
  RA_K_OBJ_POS, RA_K_OBJ_REL_POS, RA_K_OBJ_VEL_POS, RA_K_OBJ_ROT, RA_K_OBJ_VEL_ROT, RA_K_ROBOT_JOINT_POS, RA_K_GRIPPER_POS, RA_K_GRIPPER_VELP, RA_K_GRIPPER_CONTROLS,
  RA_K_GRIPPER_QPOS, RA_K_GRIPPER_VEL, RA_K_QPOS, RA_K_QPOS_GOAL, RA_K_GOAL_OBJ_POS, RA_K_GOAL_OBJ_ROT, RA_K_IS_GOAL_ACHIEVED, RA_K_REL_GOAL_OBJ_POS,
  RA_K_REL_GOAL_OBJ_ROT, RA_K_OBJ_GRIPPER_CONTACT, RA_K_OBJ_BBOX_SIZE, RA_K_OBJ_COLORS, RA_K_SAFETY_STOP, RA_K_TCP_FORCE, RA_K_TCP_TORQUE,
  RA_K_MASK_FIRST,      // the end of the row without mask_obs; the keys of mask_obs follow
  RA_K_PLACEMENT_MASK = RA_K_MASK_FIRST, RA_K_GOAL_PLACEMENT_MASK, RA_K_MASKED_GOAL_OBJ_POS, RA_K_MASKED_GOAL_OBJ_ROT, RA_K_MASKED_REL_GOAL_OBJ_POS,
  RA_K_MASKED_REL_GOAL_OBJ_ROT, RA_K_MASKED_OBJ_POS, RA_K_MASKED_OBJ_ROT, RA_K_MASKED_OBJ_REL_POS, RA_K_MASKED_OBJ_VEL_POS, RA_K_MASKED_OBJ_VEL_ROT,
  RA_K_MASKED_OBJ_GRIPPER_CONTACT, RA_K_MASKED_OBJ_BBOX_SIZE, RA_K_MASKED_OBJ_COLORS,
  RA_K_END
};
struct RaWidth { int n, c, q; };      // n * num_objects + c + q * nq scalars
constexpr RaWidth ra_key_width(int key) {
  switch (key) {
    case RA_K_ROBOT_JOINT_POS: return {0, 6, 0};
    case RA_K_GRIPPER_POS: case RA_K_GRIPPER_VELP: case RA_K_TCP_FORCE: case RA_K_TCP_TORQUE: return {0, 3, 0};
    case RA_K_GRIPPER_CONTROLS: case RA_K_GRIPPER_QPOS: case RA_K_GRIPPER_VEL: case RA_K_IS_GOAL_ACHIEVED: case RA_K_SAFETY_STOP: return {0, 1, 0};
    case RA_K_QPOS: case RA_K_QPOS_GOAL: return {0, 0, 1};
    case RA_K_PLACEMENT_MASK: case RA_K_GOAL_PLACEMENT_MASK: return {1, 0, 0};
    case RA_K_OBJ_GRIPPER_CONTACT: case RA_K_MASKED_OBJ_GRIPPER_CONTACT: return {2, 0, 0};
    case RA_K_OBJ_COLORS: case RA_K_MASKED_OBJ_COLORS: return {4, 0, 0};
    default: return {3, 0, 0};      // positions, rotations, velocities, bounding boxes: three per object
  }
}
constexpr RaWidth ra_keys_before(int key) {
  RaWidth s = {0, 0, 0};
  for (int k = 0; k < key; k++) { const RaWidth w = ra_key_width(k); s.n += w.n; s.c += w.c; s.q += w.q; }
  return s;
}
// column of KEY's first scalar in a row of N objects and nq qpos entries (KEY = RA_K_MASK_FIRST / RA_K_END: the row's width without / with mask_obs)
template <int KEY>
__host__ __device__ inline int ra_key_offset(int N, int nq) { constexpr RaWidth s = ra_keys_before(KEY); return s.n * N + s.c + s.q * nq; }
__host__ __device__ inline int ra_row_width(int N, int nq, int mask_obs) { return mask_obs ? ra_key_offset<RA_K_END>(N, nq) : ra_key_offset<RA_K_MASK_FIRST>(N, nq); }
}  // namespace rgb
