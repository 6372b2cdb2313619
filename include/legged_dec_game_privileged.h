/*
 * legged_dec_game_privileged.h -- C-ABI of the privileged (critic-only) observations of the decentralised predator-prey game
 * (task `dec_high_level_game`).
 *
 * The prey senses the predator inside a 64 degree field of view only; a critic that reads the same 16 occluded numbers values a predator
 * two metres behind the robot like one thirty metres away.  The critic exists during training only, so it may read the simulator's state:
 * one launch behind whichever post launch ran (lg_dec_game_post, lg_dec_outcome_post, lg_dec_member_outcome_post) writes one row per env
 * for either agent's critic, from the state that launch left -- after its resets, the instant the observations belong to:
 *
 *     lg_dec_game_act (or lg_dec_game_pre + the actors) -> lg_step -> lg_dec_*_post -> lg_dec_game_privileged_obs
 *
 * With p = predator_pos[e], q = ll_root_states[e, 0:3], v = ll_root_states[e, 7:10], (fx, fy) the yaw-forward vector of the prey exactly
 * as the visibility test of the post stage forms it, L = params.max_episode_length and clock = (L - episode_length_buf[e]) / L, correctly
 * rounded, not clamped (1 at the start of an episode, 0 in the step whose successor times out):
 *
 *     prey critic      [0:16] obs_prey[e]   [16:19] p - q   [19:21] fx, fy   [21] clock
 *     predator critic  [0:3]  obs_pred[e]   [3:5] fx, fy    [5:8] v          [8] obs_prey[e, 15] (the prey sees the predator now)   [9] clock
 *
 * The clock reads episode_length_buf, which is what the game's time-out tests and what a runner randomises at start (curr_episode_step is
 * neither).  The reference allocates a zero buffer for these fields and never fills it; the layouts are defined here.
 *
 * A library of its own (liblegged_dec_game_privileged.so): it reads the two structs of legged_dec_game.h and nothing else of the other
 * libraries.  Conventions as in legged_hip.h: extern "C", 0 = success, negative = error (text via lg_dec_game_privileged_last_error()).
 */
#ifndef LEGGED_DEC_GAME_PRIVILEGED_H
#define LEGGED_DEC_GAME_PRIVILEGED_H

#include "legged_dec_game.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LG_DEC_NUM_PRIV_PREY 22   /* the prey's observations, p - q, fx, fy, clock */
#define LG_DEC_NUM_PRIV_PRED 10   /* the predator's observations, fx, fy, v, the prey's visibility flag, clock */

/* One thread per env.  Read: params->num_envs and max_episode_length; buffers->predator_pos, ll_root_states, obs_prey, obs_pred,
 * episode_length_buf as the post launch left them.  Written: priv_pred [N,10] and priv_prey [N,22], each may be NULL (that agent's critic
 * reads its plain observations) and nothing else.  Errors: -1 a null argument or buffer, or both destinations NULL (nothing is launched);
 * -2 num_envs < 1 or max_episode_length < 1; -10 a HIP error. */
int lg_dec_game_privileged_obs(const lg_dec_game_params *params, const lg_dec_game_buffers *buffers, float *priv_pred, float *priv_prey,
                               void *stream);

const char *lg_dec_game_privileged_last_error(void);

/* sizeof of 0: lg_dec_game_params, 1: lg_dec_game_buffers (layout check of the binding); -1 otherwise */
int lg_dec_game_privileged_sizeof(int which);

#ifdef __cplusplus
}
#endif
#endif
