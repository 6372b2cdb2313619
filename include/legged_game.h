/*
 * legged_game.h -- C-ABI of the predator-prey game layer (task `high_level_game`).
 *
 * The game wraps a low-level locomotion env (the `a1` task, legged_hip.h) and adds a kinematic predator.  One
 * high-level step of the reference (legged_gym/envs/a1_game/high_level_game.py:146-241) is five launches with no
 * host in between:  high-level actor -> lg_game_pre -> low-level actor -> lg_step -> lg_game_post,
 * or three:  lg_game_act (both actors and the clip) -> lg_step -> lg_game_post.
 *
 * The entry points are stateless: the parameters travel by value in the kernel arguments and the buffers are raw
 * device pointers owned by the caller.  They stand in for the gym calls
 *   set_actor_root_state_tensor            high_level_game.py:263,287   (predator integration)
 *   set_actor_root_state_tensor_indexed    low_level_game.py:442-451    (root-state reset of prey and predator)
 * and the torch arithmetic around them.  They are product-only (the CPU oracle has no game layer) and therefore live in
 * this header, not in legged_hip.h.  LG_ABI_VERSION is unaffected.
 *
 * Conventions as in legged_hip.h: extern "C", 0 = success, negative = error (text via lg_last_error()).
 */
#ifndef LEGGED_GAME_H
#define LEGGED_GAME_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LG_GAME_NUM_OBS      19   /* 4 x sensed relative predator position, 4 visibility flags, prey position relative to the predator */
#define LG_GAME_NUM_ACTIONS  6    /* prey command (lin_vel_x, lin_vel_y, ang_vel_yaw, heading) + predator velocity (vx, vy) */

typedef struct lg_game_params {
    int32_t  num_envs, decimation, heading_command, only_positive_rewards;
    int32_t  custom_origins, _pad0;
    uint64_t seed;                                   /* Philox key, as lg_params.seed */
    float    cmd_lin_vel_x[2], cmd_lin_vel_y[2];     /* clip ranges of command[:, 0:2]  (:162-163) */
    float    predator_lin_vel_x[2], predator_lin_vel_y[2];   /* clip ranges of command[:, 4:6]  (:168-169) */
    float    capture_dist;                           /* env.capture_dist (:198) */
    float    env_radius;                             /* env.env_radius, < 0 = None (:205-219) */
    float    half_fov;                               /* 1.20428 / 2 (:427) */
    float    max_rel_pos;                            /* MAX_REL_POS = 100 (:55, :345-347) */
    float    ll_rew_weight;                          /* 2.0 (:364) */
    float    scale_evasion_dt, scale_pursuit_dt;     /* rewards.scales.* x ll_env.dt (:547) */
    float    sim_dt;                                 /* ll_env.cfg.sim.dt (:282) */
    float    predator_z, _pad1;                      /* 0.3 (low_level_game.py:432) */
    float    base_init_state[13];  float _pad2;      /* pos, quat xyzw, lin vel, ang vel of the prey */
} lg_game_params;

typedef struct lg_game_buffers {
    float         *command;             /* [N,6]  in: the policy's output; out: clipped / wrapped (lg_game_pre) */
    /* buffers of the low-level env (legged_hip.h: lg_buffers) */
    float         *ll_root_states;      /* [N,13] read; rows of done envs rewritten by lg_game_post */
    float         *ll_commands;         /* [N,4]  written by lg_game_pre */
    const float   *ll_env_origins;      /* [N,3] */
    const float   *ll_rew_buf;          /* [N]    reward of the preceding lg_step */
    const uint8_t *ll_reset_buf;        /* [N]    resets of the preceding lg_step */
    const int64_t *ll_step_counter;     /* [1]    read when common_step_counter = -1 */
    /* the game's own state */
    float         *predator_pos;        /* [N,3] */
    float         *obs;                 /* [N,19] read (history) and rewritten in place */
    float         *rew;                 /* [N] */
    uint8_t       *reset_buf;           /* [N] */
    int64_t       *curr_episode_step;   /* [N] */
    int64_t       *episode_length_buf;  /* [N] */
    float         *episode_sums;        /* [2,N]: evasion, pursuit (dir() order) */
} lg_game_buffers;

/* high_level_game.py:162-174: clip command[:, 0:2] and [:, 4:6], wrap column 2 to (-pi, pi] under heading_command (the reference wraps column
 * 2, not the heading column 3), write the result back and copy command[:, 0:4] to the low-level env's commands.  One thread per env. */
int lg_game_pre(const lg_game_params *params, const lg_game_buffers *buffers, void *stream);

/* high_level_game.py:182-239 in one launch, one thread per env: episode step, predator integration (:265-287), reward (:357-378), capture /
 * radius / low-level dones (:197-236), root-state reset and predator placement of the done envs (:326-349, low_level_game.py:401-451),
 * observation with the occlusion model (:380-482).  `common_step_counter` keys the reset draws (seed; env, step, RNG_GAME_ROOT = 16 /
 * RNG_GAME_PREDATOR = 17, block); -1 = read `ll_step_counter` as the preceding lg_step left it (graph replay). */
int lg_game_post(const lg_game_params *params, const lg_game_buffers *buffers, int64_t common_step_counter, void *stream);

/* Both actors of a high-level step and lg_game_pre in ONE launch, workgroups split by role (the low-level policy reads the observation the
 * previous lg_step left, so nothing in it depends on the new command):
 *   low-level role   actions = actor_ll(ll_obs), deterministic                                  = lg_policy_act(ll, ..., deterministic = 1)
 *   high-level role  sample = actor_hl(hl_obs) + std * eps; command = clip / wrap(sample)       = lg_policy_act(hl, ...) + lg_game_pre
 * Each role's results are bit-identical to those stand-alone launches.  `hl` / `ll` are lg_policy handles (legged_hip.h: lg_policy_create);
 * seed / step / step_counter / deterministic as in lg_policy_act and apply to the high-level role.  Written: buffers->command [N,6],
 * buffers->ll_commands [N,4], ll_actions [N, actions of ll], mean [N,6], and where the pointer is not NULL: sample [N,6] (the unclipped
 * sample), sigma [N,6] (the broadcast std), log_prob [N] (log N(sample; mean, std) summed over the six actions: what PPO.act stores
 * before the env clips the caller's tensor), obs_copy [N,19] (the observations the high-level role read).
 * Compiled for the 19-512-256-128-6 / 235-512-256-128 pair at wide precision 1 (lg_mlp_wide_set_precision); -4 otherwise: issue
 * lg_policy_act x 2 + lg_game_pre instead. */
struct lg_policy;
int lg_game_act(struct lg_policy *hl, struct lg_policy *ll, const lg_game_params *params, const lg_game_buffers *buffers,
                const float *hl_obs, const float *ll_obs, float *ll_actions, float *mean, uint64_t seed, int64_t step,
                const int64_t *step_counter, int32_t deterministic, float *sample, float *sigma, float *log_prob, float *obs_copy, void *stream);

/* sizeof of 0: lg_game_params, 1: lg_game_buffers (layout check of the binding); -1 otherwise */
int lg_game_sizeof(int which);

#ifdef __cplusplus
}
#endif
#endif
