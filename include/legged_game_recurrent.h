/*
 * legged_game_recurrent.h -- C-ABI of the recurrent high-level policy of the predator-prey game tasks (`high_level_game`,
 * `scripted_predator_game`): both actors of a high-level step in one launch when the high-level actor sits behind an LSTM memory.
 *
 * The policy stage of a high-level step is then two launches,
 *     lg_lstm_step (both memories, legged_recurrent.h)  ->  lg_game_lstm_act  ->  lg_step  ->  lg_game_post / lg_pursuer_post / lg_outcome_post
 * where the feed-forward policy has one (legged_game.h: lg_game_act).
 *
 * A library of its own, liblegged_game_recurrent.so: it links against nothing of liblegged_hip.so and reads the handles that library
 * created (lg_policy_create, lg_lstm_actor_create); both are built by one build from the same headers.  Conventions as in legged_game.h:
 * extern "C", stateless, parameters by value in the kernel arguments, raw device pointers owned by the caller, 0 = success,
 * negative = error with the text in lg_game_recurrent_last_error() (this library's own, per thread).
 */
#ifndef LEGGED_GAME_RECURRENT_H
#define LEGGED_GAME_RECURRENT_H

#include <stdint.h>
#include "legged_game.h"
#include "legged_recurrent.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lg_game_act for a recurrent high-level actor, workgroups split by role:
 *   low-level role   ll_actions = actor_ll(ll_obs), deterministic                      = lg_policy_act(ll, ..., deterministic = 1) at wide precision 1
 *   high-level role  sample = actor_hl(h) + std * eps; command = clip / wrap(sample)   = lg_lstm_actor_act(hl, h, ...) + lg_game_pre
 * Each role's results are bit-identical to those stand-alone launches.  `h` [N, hl->dims[0]] is the actor memory's output of this step
 * (lg_lstm_step); `hl` an lg_lstm_actor handle with six actions, `ll` the wide 235-input lg_policy handle.  seed / step / step_counter /
 * deterministic as in lg_lstm_actor_act.  Written: buffers->command [N,6], buffers->ll_commands [N,4], ll_actions [N,12], mean [N,6], and
 * where the pointer is not NULL: sample [N,6] (the unclipped sample), sigma [N,6] (the broadcast std), log_prob [N] (log N(sample; mean,
 * std) summed over the six actions), obs_copy [N,19] (a copy of hl_obs, the observations the memories read; hl_obs may be NULL otherwise).
 * The low-level role is the split-bf16 kernel: at wide precision 0 (lg_mlp_wide_set_precision, which this library cannot see) the caller
 * issues lg_lstm_actor_act + lg_game_pre + lg_policy_act instead, as it does on -4.
 * Errors, all found before any launch: -1 a null required argument (buffers->command / ll_commands included, hl_obs when obs_copy is
 * given); -2 num_envs < 1; -4 hl->dims[4] != 6 or `ll` is not the wide 235-input handle; -10 a HIP failure.
 * The first call on a device raises the kernel's dynamic LDS limit: make it outside any stream capture. */
int lg_game_lstm_act(const lg_lstm_actor *hl, struct lg_policy *ll, const lg_game_params *params, const lg_game_buffers *buffers,
                     const float *h, const float *hl_obs, const float *ll_obs, float *ll_actions, float *mean,
                     uint64_t seed, int64_t step, const int64_t *step_counter, int32_t deterministic,
                     float *sample, float *sigma, float *log_prob, float *obs_copy, void *stream);

/* the text of this thread's last error of this library */
const char *lg_game_recurrent_last_error(void);

/* sizeof as this library sees them of 0: lg_game_params, 1: lg_game_buffers, 2: lg_policy, 3: lg_lstm_actor; -1 otherwise */
int lg_game_recurrent_sizeof(int which);

#ifdef __cplusplus
}
#endif
#endif
