/*
 * legged_dec_game.h -- C-ABI of the decentralised predator-prey game (task `dec_high_level_game`).
 *
 * Two agents per env, each with its own observations, reward and policy (reference
 * legged_gym/envs/a1_game/dec_high_level_game.py): the prey is the A1 robot under a frozen low-level locomotion policy and
 * is commanded with (lin_vel_x, lin_vel_y, ang_vel_yaw, heading); the predator is a kinematic point commanded with (vx, vy).
 * One step of the reference (:169-258) is four launches with no host in between:
 *     lg_dec_game_pre -> low-level actor (lg_policy_act) -> lg_step -> lg_dec_game_post
 * or, with both agents' actors on the device, three:  lg_dec_game_act -> lg_step -> lg_dec_game_post.
 *
 * Stateless like legged_game.h: parameters by value in the kernel arguments, raw device pointers owned by the caller,
 * 0 = success, negative = error (text via lg_last_error()).  legged_game.h, legged_hip.h and LG_ABI_VERSION are unaffected.
 */
#ifndef LEGGED_DEC_GAME_H
#define LEGGED_DEC_GAME_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LG_DEC_NUM_OBS_PREY      16   /* 4 x sensed relative predator position, 4 visibility flags */
#define LG_DEC_NUM_OBS_PRED      3    /* prey position relative to the predator */
#define LG_DEC_NUM_ACTIONS_PREY  4    /* lin_vel_x, lin_vel_y, ang_vel_yaw, heading */
#define LG_DEC_NUM_ACTIONS_PRED  2    /* vx, vy */
#define LG_DEC_NUM_SUMS          3    /* episode sums / means: prey evasion, predator pursuit, prey termination */
#define LG_DEC_NUM_DOF           12

typedef struct lg_dec_game_params {
    int32_t  num_envs, decimation, heading_command, custom_origins;
    int32_t  only_positive_rewards_prey, only_positive_rewards_pred;   /* rewards_prey / rewards_predator .only_positive_rewards (:335, :355) */
    int32_t  max_episode_length, _pad0;              /* ceil(episode_length_s / ll_env.dt) (:590); time-out when episode_length_buf exceeds it (:268) */
    uint64_t seed;                                   /* Philox key, as lg_params.seed */
    float    cmd_lin_vel_x[2], cmd_lin_vel_y[2];     /* clip ranges of command_prey[:, 0:2]  (:182-183) */
    float    predator_lin_vel_x[2], predator_lin_vel_y[2];   /* clip ranges of command_pred[:, 0:2]  (:188-189) */
    float    capture_dist;                           /* env.capture_dist (:267) */
    float    half_fov;                               /* 1.20428 / 2 (:417) */
    float    max_rel_pos;                            /* MAX_REL_POS = 100 (:55, :291) */
    float    ll_rew_weight;                          /* 2.0 (:328) */
    float    scale_evasion_dt, scale_pursuit_dt;     /* rewards_prey.scales.evasion / rewards_predator.scales.pursuit x ll_env.dt (:537, :564) */
    float    scale_termination_prey_dt;              /* rewards_prey.scales.termination x ll_env.dt, 0 = absent (:338-341) */
    float    sim_dt;                                 /* ll_env.cfg.sim.dt (:229) */
    float    predator_z;                             /* 0.3 (low_level_game.py:432) */
    float    max_episode_length_s;                   /* env.episode_length_s (:589): divisor of the episode means (:301, :304) */
    float    base_init_state[13];  float _pad1;      /* pos, quat xyzw, lin vel, ang vel of the prey */
    float    default_dof_pos[LG_DEC_NUM_DOF];        /* in the joint order of the low-level dof_state buffer (low_level_game.py:391) */
} lg_dec_game_params;

typedef struct lg_dec_game_buffers {
    float         *command_prey;        /* [N,4]  in: the prey policy's output; out: clipped / wrapped (lg_dec_game_pre) */
    float         *command_pred;        /* [N,2]  in: the predator policy's output; out: clipped */
    /* buffers of the low-level env (legged_hip.h: lg_buffers) */
    float         *ll_root_states;      /* [N,13] read; rows of done envs rewritten by lg_dec_game_post */
    float         *ll_dof_state;        /* [N,12,2] (pos, vel); rows of done envs rewritten by lg_dec_game_post */
    float         *ll_commands;         /* [N,4]  written by lg_dec_game_pre */
    const float   *ll_env_origins;      /* [N,3] */
    const float   *ll_rew_buf;          /* [N]    reward of the preceding lg_step */
    const uint8_t *ll_reset_buf;        /* [N]    resets of the preceding lg_step */
    const int64_t *ll_step_counter;     /* [1]    read when common_step_counter = -1 */
    /* the game's own state */
    float         *predator_pos;        /* [N,3] */
    float         *obs_prey;            /* [N,16] read (history) and rewritten in place */
    float         *obs_pred;            /* [N,3]  written */
    float         *rew_prey, *rew_pred; /* [N] each */
    uint8_t       *reset_buf;           /* [N] */
    uint8_t       *time_out_buf;        /* [N] */
    int64_t       *curr_episode_step;   /* [N] */
    int64_t       *episode_length_buf;  /* [N] */
    float         *episode_sums;        /* [3,N]: prey evasion, predator pursuit, prey termination; rows of done envs zeroed */
    float         *episode_means;       /* [3]   the same order: mean over this launch's done envs / max_episode_length_s; untouched when none was done */
    float         *extras_accum;        /* [4]   count + three sums across workgroups; zero before the first launch, left zero by every launch */
    uint32_t      *extras_ticket;       /* [1]   workgroup ticket; zero before the first launch, left zero by every launch */
} lg_dec_game_buffers;

/* dec_high_level_game.py:182-195: clip command_prey[:, 0:2] and command_pred[:, 0:2], wrap command_prey[:, 2] to (-pi, pi] under
 * heading_command, in place, and copy command_prey to the low-level env's commands.  One thread per env. */
int lg_dec_game_pre(const lg_dec_game_params *params, const lg_dec_game_buffers *buffers, void *stream);

/* dec_high_level_game.py:228-230 + :236-258 in one launch, one thread per env: both counters, predator integration, capture / time-out
 * (:263-269), prey and predator rewards with their episode sums (:321-362), OR with the low-level resets, reset of the done envs
 * (:271-311: joints, root state, predator placement, prey history, counters, episode means), both observations (:364-392, :408-472).
 * `common_step_counter` keys the reset draws (seed; env, step, purpose, block) with the purposes RNG_GAME_ROOT = 16 and
 * RNG_GAME_PREDATOR = 17 of lg_game_post and RNG_GAME_DOF = 18 for the joints (joint j: block j >> 2, lane j & 3);
 * -1 = read `ll_step_counter` as the preceding lg_step left it (graph replay). */
int lg_dec_game_post(const lg_dec_game_params *params, const lg_dec_game_buffers *buffers, int64_t common_step_counter, void *stream);

/* optional per-agent outputs of lg_dec_game_act; the struct pointer and every member may be NULL */
typedef struct lg_dec_act_outputs {
    float *sample;      /* [N, actions] the unclipped sample */
    float *sigma;       /* [N, actions] the broadcast std */
    float *log_prob;    /* [N] log N(sample; mean, std) summed over the agent's actions: what PPO.act stores before the env clips the caller's tensor */
    float *obs_copy;    /* [N, observations] the observations the agent's role read */
} lg_dec_act_outputs;

/* The three actors of a step and lg_dec_game_pre in ONE launch, workgroups split by role:
 *   low-level role  ll_actions = actor_ll(ll_obs), deterministic                                   = lg_policy_act(ll, ..., deterministic = 1)
 *   prey role       sample = actor_prey(prey_obs) + std * eps; command_prey = clip / wrap(sample)  = lg_policy_act(prey, ...) + the prey half of lg_dec_game_pre
 *   predator role   sample = actor_pred(pred_obs) + std * eps; command_pred = clip(sample)         = lg_policy_act(pred, ...) + the predator half
 * Each role's results are bit-identical to those stand-alone launches.  `pred` / `prey` / `ll` are lg_policy handles (legged_hip.h:
 * lg_policy_create); step / step_counter as in lg_policy_act, shared by the roles.  The two sampled roles draw their noise under the same
 * purposes, so seed_pred and seed_prey must differ.  Written: buffers->command_prey [N,4], buffers->command_pred [N,2],
 * buffers->ll_commands [N,4], ll_actions [N, actions of ll], mean_prey [N,4], mean_pred [N,2] and the optional outputs.
 * Compiled for the 3-512-256-128-2 / 16-512-256-128-4 / 235-512-256-128 triple at wide precision 1 (lg_mlp_wide_set_precision); -4
 * otherwise, with nothing launched: issue lg_policy_act x 3 + lg_dec_game_pre instead. */
struct lg_policy;
int lg_dec_game_act(struct lg_policy *pred, struct lg_policy *prey, struct lg_policy *ll, const lg_dec_game_params *params,
                    const lg_dec_game_buffers *buffers, const float *pred_obs, const float *prey_obs, const float *ll_obs, float *ll_actions,
                    float *mean_pred, float *mean_prey, uint64_t seed_pred, uint64_t seed_prey, int64_t step, const int64_t *step_counter,
                    int32_t deterministic_pred, int32_t deterministic_prey, const lg_dec_act_outputs *out_pred, const lg_dec_act_outputs *out_prey,
                    void *stream);

/* sizeof of 0: lg_dec_game_params, 1: lg_dec_game_buffers, 2: lg_dec_act_outputs (layout check of the binding); -1 otherwise */
int lg_dec_game_sizeof(int which);

#ifdef __cplusplus
}
#endif
#endif
