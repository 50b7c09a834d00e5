// rg_env_common.h — the episode bookkeeping the env post-step kernels share (rg_env_kernel.h, rb_env_kernel.h, ra_env_kernel.h): the counter-based
// generator, MultiGoalTracker, the pipelined reset recipe's phase machine and MjSim.reset as row writes, each stated once.  Plain functions on plain pointers
// and scalars: the C-ABI argument structs stay with their kernels, and so does everything the kernels do differently (their call sites say what).
#pragma once
#include "rg_types.h"

// ---- counter-based generator: one 32-bit hash per (seed, step, env, k)
__device__ __forceinline__ unsigned env_hash(unsigned a, unsigned b, unsigned c, unsigned d) {
  unsigned h = a * 0x9E3779B1u ^ (b + 0x7F4A7C15u) * 0x85EBCA77u;
  h ^= h >> 15; h *= 0xC2B2AE3Du; h ^= (c + 0x165667B1u) * 0x27D4EB2Fu; h ^= h >> 13; h *= 0x9E3779B1u;
  h ^= (d + 0xD6E8FEB8u) * 0x85EBCA77u; h ^= h >> 16; h *= 0xC2B2AE3Du; h ^= h >> 15; h *= 0x27D4EB2Fu; h ^= h >> 13;
  return h;
}
__device__ __forceinline__ float env_u01(unsigned seed, unsigned step, unsigned e, unsigned k) { return (float)(env_hash(seed, step, e, k) >> 8) * (1.0f / 16777216.0f); }   // [0, 1)
__device__ __forceinline__ float env_normal(unsigned seed, unsigned step, unsigned e, unsigned k_u1, unsigned k_u2) {   // Box-Muller on the uniforms of counters k_u1, k_u2
  const float u1 = fmaxf(env_u01(seed, step, e, k_u1), 1e-7f), u2 = env_u01(seed, step, e, k_u2);
  return sqrtf(-2.0f * logf(u1)) * cosf(6.2831853f * u2);
}

// ---- MultiGoalTracker.process (multi_goal_tracker.py:157-241) of env e with the envs' settings (one successful step suffices)
struct EnvTracked { bool got, trial, timeout, newgoal; int ssl; };   // flags stay bool: as int, rg_post_step_kernel reserves private memory (profiles/env_common.txt, "code objects")
__device__ __forceinline__ EnvTracked env_tracker_process(int e, int* steps, int* steps_since_last_goal, int* successes_so_far, int* consecutive, int max_timesteps_per_goal, int successes_needed, int succ) {
  EnvTracked r;
  steps[e] += 1;
  r.ssl = steps_since_last_goal[e] + 1;
  const int cons = succ ? consecutive[e] + 1 : 0;
  r.got = cons >= 1;
  if (r.got) successes_so_far[e] += 1;
  r.timeout = !r.got && r.ssl >= max_timesteps_per_goal;
  r.trial = r.got && successes_so_far[e] >= successes_needed;
  if (r.trial) r.ssl = 0;
  r.newgoal = r.got && !r.trial;
  steps_since_last_goal[e] = r.ssl; consecutive[e] = cons;
  return r;
}
// the tail of RobotEnv.reset (robot_env.py:787-792) when an episode starts: tracker.reset, the env clock, no previous goal distance
__device__ __forceinline__ void env_episode_start(int e, int* t, int* steps, int* steps_since_last_goal, int* successes_so_far, int* goals_so_far, int* consecutive, int* prev_valid) {
  steps[e] = 0; steps_since_last_goal[e] = 0; successes_so_far[e] = 0; goals_so_far[e] = 0; consecutive[e] = 0; t[e] = 0; prev_valid[e] = 0;
}
// reset_goal's counters (robot_env.py:893-909; MultiGoalTracker.reset_goal_steps)
__device__ __forceinline__ void env_reset_goal_counters(int e, int* goals_so_far, int* steps_since_last_goal, int* consecutive) { goals_so_far[e] += 1; steps_since_last_goal[e] = 0; consecutive[e] = 0; }

// ---- the pipelined reset recipe (cube_env.py:330-355) as a phase counter: 0 = live, k > 0 = k - 1 recipe steps done; n1 steps under the zero action, the state writes
// (`wiggle`), n2 - n1 steps under one random action, then on_palm: the episode starts (`ok`) or the recipe runs again (`restart`), max_pose_resets passes at most.  A
// live env whose episode ended (`done`) and an env that crashed inside the recipe restart too.  Updates *tries; the caller stores `phase`.
struct EnvRecipeStep { bool wiggle, restart, ok; int phase; };   // flags stay bool, as in EnvTracked
__device__ __forceinline__ EnvRecipeStep env_recipe_advance(int ph0, int crash, int on_palm, int done, int live, int n1, int n2, int max_pose_resets, int* tries) {
  EnvRecipeStep r;
  const int resetting = !live, ph = ph0 + resetting;
  r.wiggle = resetting && ph == n1 + 1 && !crash;
  const int finished = resetting && ph == n2 + 1 && !crash;
  r.ok = finished && (on_palm || *tries + 1 >= max_pose_resets);
  const int retry = (finished && !r.ok) || (crash && resetting);
  const int start = done && live;
  r.restart = retry || start;
  *tries = start ? 0 : *tries + retry;
  r.phase = r.restart ? 1 : (r.ok ? 0 : ph);
  return r;
}
// forward ticks of the env's NEXT step launch: env.step 3, a recipe step 1 (simulation_interface.py:176-189), 2 with the forwards after the state writes / in on_palm
__device__ __forceinline__ int env_nticks_next(int phase, int n1, int n2) { return phase == 0 ? 3 : ((phase == n1 || phase == n2) ? 2 : 1); }

// ---- MjSim.reset of one env by its wave; ctrl, and whatever else mj_resetData clears in a kernel's layout, is the caller's
__device__ __forceinline__ void env_restart_rows(int lane, float* qpos, const float* qpos0, int nq, float* qvel, float* qacc_warmstart, int nv, float* pid, int nu, float* time, uint32_t* status) {
  for (int i = lane; i < nq; i += RG_WAVE) qpos[i] = qpos0[i];
  for (int i = lane; i < nv; i += RG_WAVE) { qvel[i] = 0.f; qacc_warmstart[i] = 0.f; }
  for (int i = lane; i < 3 * nu; i += RG_WAVE) pid[i] = 0.f;
  if (lane == 0) { *time = 0.f; *status = 0; }
}
// denormalize_position_control (robot_interface.py:247-278), absolute: action in [-1, 1] -> the actuator's ctrlrange, clamped
__device__ __forceinline__ float env_ctrl_of_action(float lo, float hi, float act) { return fminf(fmaxf(0.5f * (hi + lo) + act * 0.5f * (hi - lo), lo), hi); }
