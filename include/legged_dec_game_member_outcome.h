/*
 * legged_dec_game_member_outcome.h -- C-ABI of the outcome statistics per opponent-pool member of the decentralised predator-prey game
 * (task `dec_high_level_game`).
 *
 * lg_dec_outcome_post (legged_dec_game_outcome.h) counts why the done envs' episodes ended, one set of six integers over all envs.  With an
 * opponent pool (legged_dec_game_pool.h) the envs of one 32-env block all meet the same pool member, the one the block's entry of the slot
 * table names.  The entry point of this header is lg_dec_outcome_post with one addition: the six integers are also kept per pool member.
 * Everything lg_dec_outcome_post writes -- the per-env outputs, episode_means, the pooled accum / means / totals, extras_accum and the
 * ticket left zero -- comes out bit-identical, so it can stand where that one stands:
 *
 *     lg_dec_pool_act -> lg_step -> lg_dec_member_outcome_post
 *
 * An episode is counted for the member its block has in the launch in which it ends: the launch reads the slot table, the one
 * lg_dec_pool_act reads for the pooled role, so the table may be rewritten between replays of a captured graph.  A slot outside
 * [0, count) is clamped to that range exactly as lg_dec_pool_act clamps it.
 *
 * Rows of member_accum / member_totals are pool members, columns the six counts in the order of LG_DEC_OUTCOME_NUM_COUNTS.  They are summed
 * as integers (ballot + popcount per 32-env half of a wave, by member in LDS, then at most one 64-bit atomic add per non-zero (member,
 * count) pair and workgroup), so every count is independent of the order in which the workgroups arrive, and the column sums over the
 * members are the pooled counts.  Still ONE launch and ONE ticket per workgroup (lg_dec_game_buffers.extras_ticket): the workgroup that
 * arrives last adds member_accum into member_totals and leaves member_accum zero.  A launch without a done env leaves member_totals as it is.
 *
 * Conventions as in legged_hip.h: extern "C", 0 = success, negative = error (text via lg_last_error()).  The ABI version is unaffected.
 */
#ifndef LEGGED_DEC_GAME_MEMBER_OUTCOME_H
#define LEGGED_DEC_GAME_MEMBER_OUTCOME_H

#include "legged_dec_game_outcome.h"
#include "legged_dec_game_pool.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LG_DEC_MEMBER_OUTCOME_ROWS LG_DEC_POOL_MAX      /* 16 */

typedef struct lg_dec_member_outcome_buffers {
    const int32_t *block_slot;     /* DEVICE [ceil(num_envs / 32)]: the table lg_dec_pool_act reads for the pooled role; read by the launch */
    uint64_t *member_accum;        /* [16][6] zero between launches */
    uint64_t *member_totals;       /* [16][6] running sums since the caller last zeroed them; order of LG_DEC_OUTCOME_NUM_COUNTS */
    int32_t count, _pad;           /* members in the pool; a slot outside [0, count) is clamped exactly as lg_dec_pool_act clamps it */
} lg_dec_member_outcome_buffers;

/* lg_dec_outcome_post that also keeps the six counts per pool member.  The caller allocates member_accum and member_totals zeroed and keeps
 * launches that share them on one stream.  Errors as lg_dec_outcome_post (-1 a null argument or buffer, -2 num_envs < 1, decimation < 0 or
 * max_episode_length_s <= 0, -9 step counter -1 without ll_step_counter), and -1 for a null `members` or a null pointer inside it, -2 for
 * `count` outside 1 .. LG_DEC_MEMBER_OUTCOME_ROWS.  All of them are found before anything is launched. */
int lg_dec_member_outcome_post(const lg_dec_game_params *params, const lg_dec_game_buffers *buffers, const lg_dec_outcome_buffers *outcome,
                               const lg_dec_member_outcome_buffers *members, int64_t common_step_counter, void *stream);

/* sizeof of 0: lg_dec_member_outcome_buffers (layout check of the binding); -1 otherwise */
int lg_dec_member_outcome_sizeof(int which);

#ifdef __cplusplus
}
#endif
#endif
