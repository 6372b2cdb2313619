/*
 * legged_game_outcome.h -- C-ABI of the game outcome statistics (tasks `high_level_game` and `scripted_predator_game`).
 *
 * lg_game_post (legged_game.h) and lg_pursuer_post (legged_pursuer_game.h) decide WHY an episode ends -- capture, leaving the arena, a
 * reset of the low-level env -- in registers, fold the causes into one reset_buf bit and overwrite the positions that would tell them apart.
 * The two entry points of this header are those two launches with one addition: the causes of the done envs are counted inside the launch.
 * Everything the plain entry points write comes out bit-identical, so either can stand where the plain one stands:
 *
 *     lg_game_act (or lg_game_pre + the actors) -> lg_step -> lg_outcome_post           (high_level_game)
 *     lg_game_act (or lg_game_pre + the actors) -> lg_step -> lg_outcome_pursuer_post   (scripted_predator_game)
 *
 * Flags of a done env (NOT exclusive: an env may raise several; every done env raises at least one):
 *     captured      |prey_xy - predator_xy| < capture_dist
 *     prey_out      env_radius >= 0 and the prey's distance from its env origin > env_radius
 *     predator_out  env_radius >= 0 and the predator's distance from the env origin > env_radius
 *     fell          ll_reset_buf and not ll_time_out_buf   (the low-level env terminated: the robot fell)
 *     survived      ll_reset_buf and ll_time_out_buf       (the low-level episode ran out: the prey was never caught)
 * `steps` of a done env is its post-increment curr_episode_step before it is zeroed: the number of high-level steps the episode lasted.
 *
 * Seven integers per launch, in this order everywhere: episodes (= done envs), captured, prey_out, predator_out, fell, survived, steps.
 * They are summed as integers (per wave, per workgroup, then one 64-bit atomic add per value and workgroup), so every count is independent
 * of the order in which the workgroups arrive.  The workgroup that arrives last publishes them and leaves `accum` and `ticket` zero for
 * the next launch.  A launch without a done env leaves `means` and `totals` as they are.
 *
 * Conventions as in legged_hip.h: extern "C", 0 = success, negative = error (text via lg_last_error()).  LG_ABI_VERSION is unaffected.
 */
#ifndef LEGGED_GAME_OUTCOME_H
#define LEGGED_GAME_OUTCOME_H

#include "legged_pursuer_game.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LG_OUTCOME_NUM_COUNTS 7   /* episodes, captured, prey_out, predator_out, fell, survived, steps */
#define LG_OUTCOME_NUM_MEANS  6   /* the five rates flag / episodes, then steps / episodes */

typedef struct lg_outcome_buffers {
    const uint8_t *ll_time_out_buf;   /* [N] lg_buffers.time_out_buf of the low-level env */
    uint64_t *accum;                  /* [7] episodes, captured, prey_out, predator_out, fell, survived, steps; zero between launches */
    uint32_t *ticket;                 /* [1] zero between launches */
    float    *means;                  /* [6] five rates, mean steps; of the last step in which an env was done */
    uint64_t *totals;                 /* [7] running sums since the caller last zeroed them */
} lg_outcome_buffers;

/* lg_game_post with the outcome statistics.  The caller allocates `accum`, `ticket`, `means` and `totals` zeroed and keeps launches that
 * share them on one stream.  Errors as lg_game_post: -1 a null argument or buffer (those of `outcome` included), -2 num_envs < 1 or
 * decimation < 0, -9 step counter -1 without ll_step_counter. */
int lg_outcome_post(const lg_game_params *params, const lg_game_buffers *buffers, const lg_outcome_buffers *outcome,
                    int64_t common_step_counter, void *stream);

/* lg_pursuer_post with the outcome statistics; `predator_command` [N,2] may be NULL.  Errors as lg_pursuer_post: additionally -2 for
 * max_episode_length outside 1 .. 2^20, max_lin_vel < min_lin_vel, gain <= 0. */
int lg_outcome_pursuer_post(const lg_game_params *params, const lg_pursuer_params *pursuer, const lg_game_buffers *buffers,
                            const lg_outcome_buffers *outcome, float *predator_command, int64_t common_step_counter, void *stream);

/* sizeof of 0: lg_outcome_buffers (layout check of the binding); -1 otherwise */
int lg_outcome_sizeof(int which);

#ifdef __cplusplus
}
#endif
#endif
