/*
 * legged_pursuer_game.h -- C-ABI of the scripted pursuer (task `scripted_predator_game`).
 *
 * The task is `high_level_game` (legged_game.h) with one difference: the predator's velocity does not come from columns 4:6 of the
 * policy's command but from the reference's scripted `full_obs_predator('integrator')` (legged_gym/envs/a1_game/high_level_game.py:289-324),
 * which `step_predator_single_integrator(command=None)` (:265-287) calls: a pursuer that sees the prey at all times, heads straight for
 * it, and "loses steam" as the episode runs out.  In float32, one rounding per operation, in this order:
 *
 *     ep  = curr_episode_step + 1                       (:182 runs before the predator moves)
 *     dxy = (prey_xy - predator_xy) * gain              (:297, :307; prey_xy as the preceding lg_step left it, before this step's resets)
 *     a   = (L - ep) / L                                (:311; L = max_episode_length; the correctly rounded quotient)
 *     lim = min_lin_vel * (1 - a) + max_lin_vel * a     (:312)
 *     v   = min(max(dxy, -lim), lim)                    (:314-315, torch.clamp: lim < 0, i.e. ep > L, gives v = lim on both axes)
 *     predator_xy += sim_dt * v, `decimation` times     (:281-283)
 *
 * One high-level step is  lg_game_act (or lg_game_pre + the actors) -> lg_step -> lg_pursuer_post : lg_pursuer_post stands where
 * lg_game_post stands, on the same lg_game_params / lg_game_buffers.  Columns 4:6 of `command` are still clipped by the pre stage and are
 * then ignored, as in the reference once the `command=` argument is dropped.
 *
 * Conventions as in legged_hip.h: extern "C", 0 = success, negative = error (text via lg_last_error()).  LG_ABI_VERSION is unaffected.
 */
#ifndef LEGGED_PURSUER_GAME_H
#define LEGGED_PURSUER_GAME_H

#include "legged_game.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lg_pursuer_params {
    float   max_lin_vel;            /* speed limit at ep = 0                      2    (:301) */
    float   min_lin_vel;            /* speed limit at ep = max_episode_length     0.01 (:312) */
    float   gain;                   /* on the relative position                   2    (:307) */
    int32_t max_episode_length;     /* L = ceil(episode_length_s / low-level dt), 1 .. 2^20 */
} lg_pursuer_params;

/* lg_game_post (legged_game.h) with the predator's velocity from the rule above; everything after the integration -- reward, dones, resets,
 * predator placement, history shift, occlusion -- is lg_game_post's, with the same Philox keying.  One launch, one thread per env.
 * `predator_command` [N,2], may be NULL: receives the velocity v the kernel integrated.  `common_step_counter` = -1 reads
 * buffers->ll_step_counter.  Errors: -1 a null argument or buffer, -2 a parameter out of range (num_envs < 1, decimation < 0,
 * max_episode_length outside 1 .. 2^20, max_lin_vel < min_lin_vel, gain <= 0), -9 step counter -1 without ll_step_counter. */
int lg_pursuer_post(const lg_game_params *params, const lg_pursuer_params *pursuer, const lg_game_buffers *buffers, float *predator_command,
                    int64_t common_step_counter, void *stream);

/* sizeof of 0: lg_pursuer_params (layout check of the binding); -1 otherwise */
int lg_pursuer_sizeof(int which);

#ifdef __cplusplus
}
#endif
#endif
