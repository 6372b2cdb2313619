/*
 * legged_dec_game_recurrent.h -- C-ABI of recurrent policies on the decentralised predator-prey game (task `dec_high_level_game`): the
 * memories of both agents advanced in one launch, and the three actors of a step in one launch when both agents' actors sit behind an
 * LSTM memory.
 *
 * The policy stage of a step is then two launches,
 *     lg_dec_lstm_step (up to four memories)  ->  lg_dec_game_lstm_act  ->  lg_step  ->  lg_dec_game_post / lg_dec_outcome_post
 * where the feed-forward policies have one (legged_dec_game.h: lg_dec_game_act) and the entry points of legged_recurrent.h would need six
 * (lg_lstm_step x 2, lg_lstm_actor_act x 2, lg_dec_game_pre, lg_policy_act).
 *
 * A library of its own, liblegged_dec_game_recurrent.so: it links against nothing of the other libraries and reads the handles
 * liblegged_hip.so created (lg_lstm_create, lg_lstm_actor_create, lg_policy_create); all are built by one build from the same headers.
 * Conventions as in legged_dec_game.h: extern "C", stateless, parameters by value in the kernel arguments, raw device pointers owned by
 * the caller, 0 = success, negative = error with the text in lg_dec_game_recurrent_last_error() (this library's own, per thread).
 * The first call of either launch on a device raises its kernel's dynamic LDS limit: make it outside any stream capture.
 */
#ifndef LEGGED_DEC_GAME_RECURRENT_H
#define LEGGED_DEC_GAME_RECURRENT_H

#include <stdint.h>
#include "legged_dec_game.h"
#include "legged_recurrent.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One memory of the cell launch: lg_lstm_step's arguments of one role.  x [N, num_in of l], h_* / c_* [N, hidden of l], DEVICE, contiguous
 * float32.  l == NULL: the role is absent and its pointers are ignored. */
typedef struct lg_dec_lstm_role {
    const lg_lstm *l;
    const float   *x, *h_in, *c_in;
    float         *h_out, *c_out;
} lg_dec_lstm_role;

/* One launch advances up to four memories by one step on num_envs rows, workgroups split by role:
 *   roles[0] predator actor memory, roles[1] predator critic memory, roles[2] prey actor memory, roles[3] prey critic memory.
 * Each present role's results are bit-identical to lg_lstm_step with that role alone.  reset: [num_envs] bytes or NULL, shared by the roles;
 * a row whose flag is non-zero starts from a zero (h, c).  h_out / c_out must not alias h_in / c_in of the same role.
 * Errors, all found before anything is launched: -1 `roles` null, no present role or a null buffer of a present role; -2 num_envs < 1,
 * aliasing, or memories on different devices; -10 a HIP failure. */
int lg_dec_lstm_step(const lg_dec_lstm_role roles[4], const uint8_t *reset, int32_t num_envs, void *stream);

/* lg_dec_game_act for recurrent agents, workgroups split by role:
 *   low-level role  ll_actions = actor_ll(ll_obs), deterministic                                   = lg_policy_act(ll, ..., deterministic = 1) at wide precision 1
 *   prey role       sample = actor_prey(h_prey) + std * eps; command_prey = clip / wrap(sample)    = lg_lstm_actor_act(prey, h_prey, ...) + the prey half of lg_dec_game_pre
 *   predator role   sample = actor_pred(h_pred) + std * eps; command_pred = clip(sample)           = lg_lstm_actor_act(pred, h_pred, ...) + the predator half
 * Each role's results are bit-identical to those stand-alone launches.  `pred` / `prey` are lg_lstm_actor handles with two / four actions,
 * h_pred [N, pred->dims[0]] / h_prey [N, prey->dims[0]] the actor memories' outputs of this step (lg_dec_lstm_step), `ll` the wide 235-input
 * lg_policy handle.  step / step_counter as in lg_lstm_actor_act, shared by the roles; the two sampled roles draw their noise under the
 * same purposes, so seed_pred and seed_prey must differ.  Written: buffers->command_prey [N,4], buffers->command_pred [N,2],
 * buffers->ll_commands [N,4], ll_actions [N,12], mean_pred [N,2], mean_prey [N,4] and, per agent, the outputs whose pointer is not NULL
 * (the struct pointer may be NULL too): sample (unclipped), sigma (the broadcast std), log_prob (log N(sample; mean, std), one accumulator
 * over the agent's actions in their order), obs_copy (a copy of pred_obs [N,3] / prey_obs [N,16], the observations the memories read;
 * pred_obs / prey_obs may be NULL otherwise).
 * The low-level role is the split-bf16 kernel: at wide precision 0 (lg_mlp_wide_set_precision, which this library cannot see) the caller
 * issues lg_lstm_actor_act x 2 + lg_dec_game_pre + lg_policy_act instead, as it does on -4.
 * Errors, all found before any launch: -1 a null required argument (buffers->command_prey / command_pred / ll_commands included, an
 * agent's observations when its obs_copy is given); -2 num_envs < 1 or equal seeds; -4 pred->dims[4] != 2, prey->dims[4] != 4, a
 * max_width outside 32 .. 512 or `ll` is not the wide 235-input handle; -10 a HIP failure. */
struct lg_policy;
int lg_dec_game_lstm_act(const lg_lstm_actor *pred, const lg_lstm_actor *prey, struct lg_policy *ll, const lg_dec_game_params *params,
                         const lg_dec_game_buffers *buffers, const float *h_pred, const float *h_prey, const float *pred_obs, const float *prey_obs,
                         const float *ll_obs, float *ll_actions, float *mean_pred, float *mean_prey, uint64_t seed_pred, uint64_t seed_prey,
                         int64_t step, const int64_t *step_counter, int32_t deterministic_pred, int32_t deterministic_prey,
                         const lg_dec_act_outputs *out_pred, const lg_dec_act_outputs *out_prey, void *stream);

/* the text of this thread's last error of this library */
const char *lg_dec_game_recurrent_last_error(void);

/* sizeof as this library sees them of 0: lg_dec_game_params, 1: lg_dec_game_buffers, 2: lg_dec_act_outputs, 3: lg_policy, 4: lg_lstm_actor,
 * 5: lg_lstm, 6: lg_dec_lstm_role; -1 otherwise */
int lg_dec_game_recurrent_sizeof(int which);

#ifdef __cplusplus
}
#endif
#endif
