// lg_game_outcome_entry.h -- C entry points of the outcome statistics (include/legged_game_outcome.h).  Host code only: the kernels live in
// lg_game_outcome.hip behind launch_outcome_post.  An entry header of lg_game_entry.hip; includes what it uses.
#pragma once
#include "lg_pursuer_game.h"        // pursuer_check; with lg_game.h: fail / HIP_TRY (lg_host.h), game_check, game_post_check
#include "../../include/legged_game_outcome.h"

namespace lg {
int launch_outcome_post(bool scripted, const lg_game_params &P, const lg_pursuer_params &Q, const lg_game_buffers &B, const lg_outcome_buffers &O,
                        float *predator_command, int64_t step, void *stream);      // lg_game_outcome.hip; returns the hipError_t of the launch
}

extern "C" {

static int outcome_check(const char *who, const lg_outcome_buffers *O) {
    if (!O->ll_time_out_buf || !O->accum || !O->ticket || !O->means || !O->totals) return lg::fail(-1, "%s: a pointer of lg_outcome_buffers is null", who);
    return 0;
}

int lg_outcome_post(const lg_game_params *P, const lg_game_buffers *B, const lg_outcome_buffers *O, int64_t common_step_counter, void *stream) {
    if (!O) return lg::fail(-1, "null argument");
    if (int rc = game_check(P, B)) return rc;
    if (int rc = outcome_check("lg_outcome_post", O)) return rc;
    if (int rc = game_post_check("lg_outcome_post", B, true, common_step_counter)) return rc;
    HIP_TRY((hipError_t)lg::launch_outcome_post(false, *P, lg_pursuer_params{0.0f, 0.0f, 0.0f, 0}, *B, *O, nullptr, common_step_counter, stream));
    return 0;
}

int lg_outcome_pursuer_post(const lg_game_params *P, const lg_pursuer_params *Q, const lg_game_buffers *B, const lg_outcome_buffers *O,
                            float *predator_command, int64_t common_step_counter, void *stream) {
    if (!Q || !O) return lg::fail(-1, "null argument");
    if (int rc = game_check(P, B)) return rc;
    if (int rc = pursuer_check(Q)) return rc;
    if (int rc = outcome_check("lg_outcome_pursuer_post", O)) return rc;
    if (int rc = game_post_check("lg_outcome_pursuer_post", B, false, common_step_counter)) return rc;
    HIP_TRY((hipError_t)lg::launch_outcome_post(true, *P, *Q, *B, *O, predator_command, common_step_counter, stream));
    return 0;
}

int lg_outcome_sizeof(int which) { return which == 0 ? (int)sizeof(lg_outcome_buffers) : -1; }

}  // extern "C"
