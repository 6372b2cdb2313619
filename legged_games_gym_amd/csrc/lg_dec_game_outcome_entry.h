// lg_dec_game_outcome_entry.h -- C entry points of the decentralised game's outcome statistics (include/legged_dec_game_outcome.h).  Host
// code only: the kernel lives in lg_dec_game_outcome.hip behind launch_dec_outcome.  An entry header of lg_game_entry.hip; includes what it
// uses.
#pragma once
#include "lg_dec_game.h"            // fail / HIP_TRY (lg_host.h), dec_game_check, dec_game_post_check
#include "../../include/legged_dec_game_outcome.h"

namespace lg {
int launch_dec_outcome(const lg_dec_game_params &P, const lg_dec_game_buffers &B, const lg_dec_outcome_buffers &O, int64_t step,
                       void *stream);      // lg_dec_game_outcome.hip; returns the hipError_t of the launch
}

extern "C" {

static int dec_outcome_check(const char *who, const lg_dec_outcome_buffers *O) {      // also lg_member_outcome_entry.h
    if (!O->ll_time_out_buf || !O->accum || !O->means || !O->totals) return lg::fail(-1, "%s: a pointer of lg_dec_outcome_buffers is null", who);
    return 0;
}

int lg_dec_outcome_post(const lg_dec_game_params *P, const lg_dec_game_buffers *B, const lg_dec_outcome_buffers *O, int64_t common_step_counter, void *stream) {
    if (!O) return lg::fail(-1, "lg_dec_outcome_post: lg_dec_outcome_buffers is null");
    if (int rc = dec_game_check(P, B)) return rc;
    if (int rc = dec_outcome_check("lg_dec_outcome_post", O)) return rc;
    if (int rc = dec_game_post_check("lg_dec_outcome_post", P, B, common_step_counter)) return rc;
    HIP_TRY((hipError_t)lg::launch_dec_outcome(*P, *B, *O, common_step_counter, stream));
    return 0;
}

int lg_dec_outcome_sizeof(int which) { return which == 0 ? (int)sizeof(lg_dec_outcome_buffers) : -1; }

}  // extern "C"
