/*
 * legged_dec_game_pool.h -- C-ABI of the opponent pool of the decentralised predator-prey game (task `dec_high_level_game`).
 *
 * lg_dec_game_act (legged_dec_game.h) runs each sampled role -- prey, predator -- with ONE actor for all envs.  Training against a
 * mixture of opponents (the live one in part of the envs, frozen earlier versions in the rest) needs a role whose actor differs between
 * envs.  A role's workgroup serves 32 envs and streams its weights from global memory, so which actor it streams is decided per workgroup:
 * the entry point of this header is lg_dec_game_act with, for a role that is given a pool, the weights, biases and std of every 32-env
 * block taken from the pool member that a device table names for that block.  Still one launch; it can stand where the plain one stands:
 *
 *     lg_dec_pool_act -> lg_step -> lg_dec_game_post (or lg_dec_outcome_post)
 *
 * Per block, every result of a pooled role (command, ll_commands, mean, sample, sigma, log-prob, observation copy) is bit-identical to
 * lg_dec_game_act launched with that block's member as the role's handle, with the same seeds, step and env indices: the role body and
 * the noise keys (seed; env, step, 100 + group) are those of lg_dec_game_act, only the operands' addresses differ.
 *
 * A pool is a device table of LG_DEC_POOL_MAX rows, one per member: the addresses of the member's packed weights, biases and std.  It is
 * filled ONCE, by lg_dec_pool_create, with a synchronous copy; no later call writes it.  The rows point into the members' own buffers,
 * which lg_policy_load_device repacks in place: the pool follows such an update, also underneath a captured graph.  lg_dec_pool_create
 * allocates and copies synchronously and is therefore NOT allowed inside a stream capture.
 *
 * Conventions as in legged_hip.h: extern "C", 0 = success, negative = error (text via lg_last_error()).  The ABI version is unaffected.
 */
#ifndef LEGGED_DEC_GAME_POOL_H
#define LEGGED_DEC_GAME_POOL_H

#include "legged_dec_game.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LG_DEC_POOL_MAX 16
#define LG_DEC_POOL_BLOCK_ENVS 32                 /* envs per block of the slot tables: block b = envs 32 b .. 32 b + 31 */
typedef struct lg_dec_pool lg_dec_pool;           /* opaque; owns a device table of LG_DEC_POOL_MAX entries */

/* what lg_dec_pool_query reports */
typedef struct lg_dec_pool_info {
    int32_t count, role, device, _pad;
    const void *table;                            /* DEVICE address of the table (read-only for the caller) */
} lg_dec_pool_info;

/* role: 1 = prey (16-512-256-128-4), 2 = predator (3-512-256-128-2).  members[i] are lg_policy handles of that shape.
 * The pool does not own them.  They must outlive it and must not be re-created (lg_policy_destroy + lg_policy_create gives new buffers).
 * lg_policy_load_device repacks in place, and the pool follows it.
 * Errors, all found before anything is allocated: -1 a null argument or member, -2 count outside 1 .. LG_DEC_POOL_MAX, a role other than
 * 1 / 2 or a member on another device, -4 a member whose shape is not the role's.  -10 when the table cannot be allocated or copied.
 * Not allowed inside a stream capture. */
int lg_dec_pool_create(struct lg_policy *const *members, int32_t count, int32_t role, int32_t device, lg_dec_pool **out);
int lg_dec_pool_destroy(lg_dec_pool *pool);       /* -1 for a null pool */
int lg_dec_pool_query(const lg_dec_pool *pool, lg_dec_pool_info *info);

/* lg_dec_game_act with, for each sampled role that is given a pool, the weights, biases and std of every 32-env block b taken from
 * member block_slot[b] of that pool.
 * block_slot_*: DEVICE int32 [ceil(num_envs / 32)], read by the launch, so it may be rewritten between replays of a captured graph.  A
 * value outside [0, count) is clamped to that range by the kernel.  A role without a pool (NULL, NULL) uses its handle as
 * lg_dec_game_act does.  With a pool, the handle argument of that role is ignored and may be NULL.
 * Errors as lg_dec_game_act, all found before anything is launched: -1 a null argument (a pool given without its slot table included),
 * -2 num_envs < 1, decimation < 0 or seed_pred == seed_prey, -4 wide precision != 1 (lg_mlp_wide_set_precision), a handle whose shape
 * is not its role's or a pool created for the other role: nothing is launched; issue one lg_policy_act per member in use on all envs,
 * select the rows by block, then lg_dec_game_pre. */
int lg_dec_pool_act(struct lg_policy *pred, struct lg_policy *prey, struct lg_policy *ll, const lg_dec_pool *pool_pred,
                    const int32_t *block_slot_pred, const lg_dec_pool *pool_prey, const int32_t *block_slot_prey,
                    const lg_dec_game_params *params, const lg_dec_game_buffers *buffers, const float *pred_obs, const float *prey_obs,
                    const float *ll_obs, float *ll_actions, float *mean_pred, float *mean_prey, uint64_t seed_pred, uint64_t seed_prey,
                    int64_t step, const int64_t *step_counter, int32_t deterministic_pred, int32_t deterministic_prey,
                    const lg_dec_act_outputs *out_pred, const lg_dec_act_outputs *out_prey, void *stream);

/* sizeof of 0: lg_dec_pool_info (layout check of the binding); -1 otherwise */
int lg_dec_pool_sizeof(int which);

#ifdef __cplusplus
}
#endif
#endif
