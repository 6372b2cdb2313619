/*
 * legged_dec_pool_recurrent.h -- C-ABI of the opponent pool for recurrent policies on the decentralised predator-prey game (task
 * `dec_high_level_game`).
 *
 * legged_dec_game_recurrent.h runs each agent's actor memory and actor MLP with ONE set of weights for all envs.  Training a recurrent
 * learner against a mixture of opponents (the live one in part of the envs, frozen earlier versions in the rest) needs a role whose
 * weights differ between envs.  A workgroup of the cell launch and of a sampled role of the actor launch serves 32 env rows and streams its
 * weights from global memory, so which member's weights it streams is decided per workgroup.  The two launches of this header are
 * lg_dec_lstm_step and lg_dec_game_lstm_act with, for a role that is given a pool, the packed weights of every 32-env block taken from the
 * pool member that a device table names for that block.  They stand where the plain ones stand:
 *
 *     lg_dec_pool_lstm_step  ->  lg_dec_pool_lstm_act  ->  lg_step  ->  lg_dec_game_post (or an outcome post)
 *
 * Per block, every value a pooled role writes (h, c; command, ll_commands, mean, sample, sigma, log-prob, observation copy) is
 * bit-identical to lg_dec_lstm_step / lg_dec_game_lstm_act launched with that block's member as the role's handle, with the same seeds,
 * step and env indices: the cell, the actor chain and the noise keys are those of the plain launches, only the operands' addresses differ.
 * A role without a pool is bit-identical to the plain launch.  A pooled role has ONE (h, c) state: which member advances a block's rows
 * is the slot table's business, and whether a state produced under one member may be continued under another is the caller's.
 *
 * A pool is a device table of LG_DEC_POOL_MAX rows of four addresses, one row per member: the packed weights and bias of the member's
 * ACTOR memory (lg_lstm) and the packed parameters and std of its actor MLP (lg_lstm_actor).  It is filled ONCE, by lg_dec_rpool_create,
 * with a synchronous copy; no later call writes it.  The rows point into the members' own buffers, which lg_lstm_load_device and
 * lg_lstm_actor_load_device repack in place: the pool follows such an update, also underneath a captured graph.  lg_dec_rpool_create
 * allocates and copies synchronously and is therefore NOT allowed inside a stream capture.  Critic memories are never pooled.
 *
 * A library of its own, liblegged_dec_pool_recurrent.so: it links against nothing of the other libraries and reads the handles
 * liblegged_hip.so created (lg_lstm_create, lg_lstm_actor_create, lg_policy_create); all are built by one build from the same headers.
 * Conventions as in legged_dec_game_recurrent.h: extern "C", 0 = success, negative = error with the text in
 * lg_dec_pool_recurrent_last_error() (this library's own, per thread).  The first call of either launch on a device raises its kernel's
 * dynamic LDS limit: make it outside any stream capture.
 */
#ifndef LEGGED_DEC_POOL_RECURRENT_H
#define LEGGED_DEC_POOL_RECURRENT_H

#include <stdint.h>
#include "legged_dec_game_recurrent.h"
#include "legged_dec_game_pool.h"                 /* LG_DEC_POOL_MAX, LG_DEC_POOL_BLOCK_ENVS */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lg_dec_rpool lg_dec_rpool;         /* opaque; owns a device table of LG_DEC_POOL_MAX rows */

/* what lg_dec_rpool_query reports: the pool and the shape every member has (member 0's) */
typedef struct lg_dec_rpool_info {
    int32_t count, role, device;
    int32_t num_in, hidden, ksteps;               /* the actor memory */
    int32_t dims[5], max_width;                   /* the actor MLP */
    const void *table;                            /* DEVICE address of the table (read-only for the caller) */
} lg_dec_rpool_info;

/* role: 1 = prey (16 inputs, 4 actions), 2 = predator (3 inputs, 2 actions).  lstm_members[i] / actor_members[i]: the ACTOR memory and the
 * actor MLP of member i.  The pool remembers member 0's shape (num_in, hidden, ksteps; dims, pad, w_off, b_off, max_width) and every
 * member must have exactly that shape.  The pool does not own the members.  They must outlive it and must not be re-created;
 * lg_lstm_load_device / lg_lstm_actor_load_device repack in place, and the pool follows them.  Rows past `count` repeat row 0.
 * Errors, all found before anything is allocated: -1 a null argument or member; -2 count outside 1 .. LG_DEC_POOL_MAX, a role other than
 * 1 / 2 or a member on another device; -4 a member whose shape differs from member 0's or is not the role's (inputs, actions, the actor's
 * input width = the memory's units).  -10 a HIP failure (the table cannot be allocated or copied).  Not allowed inside a stream capture. */
int lg_dec_rpool_create(const lg_lstm *const *lstm_members, const lg_lstm_actor *const *actor_members, int32_t count, int32_t role, int32_t device,
                        lg_dec_rpool **out);
int lg_dec_rpool_destroy(lg_dec_rpool *pool);     /* -1 for a null pool */
int lg_dec_rpool_query(const lg_dec_rpool *pool, lg_dec_rpool_info *info);

/* lg_dec_lstm_step with, for each ACTOR-memory role (roles[0] predator, roles[2] prey) that is given a pool, the packed weights and bias
 * of every 32-env block b taken from member block_slot[b] of that pool.
 * block_slot_*: DEVICE int32 [ceil(num_envs / 32)], read by the launch, so it may be rewritten between replays of a captured graph.  A
 * value outside [0, count) is clamped to that range by the kernel.  A pooled role is present whatever its `l`: the handle is ignored and
 * may be NULL, the shape comes from the pool; its buffers are required.  A role without a pool (NULL, NULL) is lg_dec_lstm_step's.
 * The critic memories (roles[1], roles[3]) are never pooled.
 * Errors as lg_dec_lstm_step, all found before anything is launched: -1 also for a pool given without its slot table; -2 also for a pool
 * on another device than the memories; -4 a pool created for the other role. */
int lg_dec_pool_lstm_step(const lg_dec_lstm_role roles[4], const lg_dec_rpool *pool_pred, const int32_t *block_slot_pred,
                          const lg_dec_rpool *pool_prey, const int32_t *block_slot_prey, const uint8_t *reset, int32_t num_envs, void *stream);

/* lg_dec_game_lstm_act with, for each sampled role that is given a pool, the packed parameters and std of every 32-env block b taken from
 * member block_slot[b] of that pool.  The low-level role is unchanged; seeds, step and noise keys are those of the plain launch.  With a
 * pool, the handle argument of that role is ignored and may be NULL.
 * Errors as lg_dec_game_lstm_act, all found before anything is launched: -1 also for a pool given without its slot table; -4 also for a
 * pool created for the other role (nothing is launched: issue lg_lstm_actor_act per member in use on all envs, select the rows by block,
 * then lg_dec_game_pre and the low-level lg_policy_act). */
int lg_dec_pool_lstm_act(const lg_lstm_actor *pred, const lg_lstm_actor *prey, struct lg_policy *ll, const lg_dec_rpool *pool_pred,
                         const int32_t *block_slot_pred, const lg_dec_rpool *pool_prey, const int32_t *block_slot_prey,
                         const lg_dec_game_params *params, const lg_dec_game_buffers *buffers, const float *h_pred, const float *h_prey,
                         const float *pred_obs, const float *prey_obs, const float *ll_obs, float *ll_actions, float *mean_pred, float *mean_prey,
                         uint64_t seed_pred, uint64_t seed_prey, int64_t step, const int64_t *step_counter, int32_t deterministic_pred,
                         int32_t deterministic_prey, const lg_dec_act_outputs *out_pred, const lg_dec_act_outputs *out_prey, void *stream);

/* the text of this thread's last error of this library */
const char *lg_dec_pool_recurrent_last_error(void);

/* sizeof as this library sees them of 0: lg_dec_game_params, 1: lg_dec_game_buffers, 2: lg_dec_act_outputs, 3: lg_policy, 4: lg_lstm_actor,
 * 5: lg_lstm, 6: lg_dec_lstm_role, 7: lg_dec_rpool_info; -1 otherwise */
int lg_dec_pool_recurrent_sizeof(int which);

#ifdef __cplusplus
}
#endif
#endif
