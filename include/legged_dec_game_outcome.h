/*
 * legged_dec_game_outcome.h -- C-ABI of the outcome statistics of the decentralised predator-prey game (task `dec_high_level_game`).
 *
 * lg_dec_game_post (legged_dec_game.h) decides WHY an episode ends -- capture, the game's own time-out, a reset of the low-level env -- in
 * registers, folds the causes into one reset_buf bit and overwrites the positions that would tell them apart.  The entry point of this
 * header is that launch with one addition: the causes of the done envs are counted inside the launch.  Everything the plain entry point
 * writes per env comes out bit-identical, so it can stand where the plain one stands:
 *
 *     lg_dec_game_act (or lg_dec_game_pre + the actors) -> lg_step -> lg_dec_outcome_post
 *
 * Flags of a done env (NOT exclusive: an env may raise several; every done env raises at least one):
 *     captured      |prey_xy - predator_xy| < capture_dist
 *     timed_out     episode_length_buf > max_episode_length: the game's own time-out, the predator failed in time
 *     fell          ll_reset_buf and not ll_time_out_buf   (the low-level env terminated: the robot fell)
 *     ll_timed_out  ll_reset_buf and ll_time_out_buf       (the low-level episode ran out)
 * `steps` of a done env is its post-increment curr_episode_step before it is zeroed: the number of high-level steps the episode lasted
 * (episode_length_buf is not used: a runner may randomise it at start).
 *
 * Six integers per launch, in this order everywhere: episodes (= done envs), captured, timed_out, fell, ll_timed_out, steps.  They are
 * summed as integers (per wave, per workgroup, then one 64-bit atomic add per non-zero value and workgroup), so every count is independent
 * of the order in which the workgroups arrive.  The launch draws ONE ticket per workgroup, lg_dec_game_buffers.extras_ticket, for the
 * episode means of lg_dec_game_post and for these counts alike; the workgroup that arrives last publishes both and leaves `accum`,
 * `extras_accum` and the ticket zero for the next launch.  A launch without a done env leaves `means` and `totals` as they are.
 *
 * Conventions as in legged_hip.h: extern "C", 0 = success, negative = error (text via lg_last_error()).  The ABI version is unaffected.
 */
#ifndef LEGGED_DEC_GAME_OUTCOME_H
#define LEGGED_DEC_GAME_OUTCOME_H

#include "legged_dec_game.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LG_DEC_OUTCOME_NUM_COUNTS 6   /* episodes, captured, timed_out, fell, ll_timed_out, steps */
#define LG_DEC_OUTCOME_NUM_MEANS  5   /* the four rates flag / episodes, then steps / episodes */

typedef struct lg_dec_outcome_buffers {
    const uint8_t *ll_time_out_buf;   /* [N] lg_buffers.time_out_buf of the low-level env */
    uint64_t *accum;                  /* [6] episodes, captured, timed_out, fell, ll_timed_out, steps; zero between launches */
    float    *means;                  /* [5] four rates, mean steps; of the last step in which an env was done */
    uint64_t *totals;                 /* [6] running sums since the caller last zeroed them */
} lg_dec_outcome_buffers;

/* lg_dec_game_post with the outcome statistics.  The caller allocates `accum`, `means` and `totals` zeroed and keeps launches that share
 * them on one stream.  Errors as lg_dec_game_post: -1 a null argument or buffer (those of `outcome` included), -2 num_envs < 1,
 * decimation < 0 or max_episode_length_s <= 0, -9 step counter -1 without ll_step_counter. */
int lg_dec_outcome_post(const lg_dec_game_params *params, const lg_dec_game_buffers *buffers, const lg_dec_outcome_buffers *outcome,
                        int64_t common_step_counter, void *stream);

/* sizeof of 0: lg_dec_outcome_buffers (layout check of the binding); -1 otherwise */
int lg_dec_outcome_sizeof(int which);

#ifdef __cplusplus
}
#endif
#endif
