// lg_member_outcome_entry.h -- C entry points of the decentralised game's outcome statistics per pool member
// (include/legged_dec_game_member_outcome.h).  Host code only: the kernel lives in lg_member_outcome.hip behind launch_member_outcome.
// An entry header of lg_game_entry.hip; includes what it uses.
#pragma once
#include "lg_dec_game_outcome_entry.h"     // dec_outcome_check; with lg_dec_game.h: fail / HIP_TRY (lg_host.h), dec_game_check, dec_game_post_check
#include "../../include/legged_dec_game_member_outcome.h"

namespace lg {
int launch_member_outcome(const lg_dec_game_params &P, const lg_dec_game_buffers &B, const lg_dec_outcome_buffers &O,
                          const lg_dec_member_outcome_buffers &M, int64_t step, void *stream);      // lg_member_outcome.hip; returns the hipError_t of the launch
}

extern "C" {

int lg_dec_member_outcome_post(const lg_dec_game_params *P, const lg_dec_game_buffers *B, const lg_dec_outcome_buffers *O,
                               const lg_dec_member_outcome_buffers *M, int64_t common_step_counter, void *stream) {
    if (!O) return lg::fail(-1, "lg_dec_member_outcome_post: lg_dec_outcome_buffers is null");
    if (!M) return lg::fail(-1, "lg_dec_member_outcome_post: lg_dec_member_outcome_buffers is null");
    if (int rc = dec_game_check(P, B)) return rc;
    if (int rc = dec_outcome_check("lg_dec_member_outcome_post", O)) return rc;
    if (!M->block_slot || !M->member_accum || !M->member_totals) return lg::fail(-1, "lg_dec_member_outcome_post: a pointer of lg_dec_member_outcome_buffers is null");
    if (M->count < 1 || M->count > LG_DEC_MEMBER_OUTCOME_ROWS) return lg::fail(-2, "lg_dec_member_outcome_post: count must be 1 .. LG_DEC_MEMBER_OUTCOME_ROWS");
    if (int rc = dec_game_post_check("lg_dec_member_outcome_post", P, B, common_step_counter)) return rc;
    HIP_TRY((hipError_t)lg::launch_member_outcome(*P, *B, *O, *M, common_step_counter, stream));
    return 0;
}

int lg_dec_member_outcome_sizeof(int which) { return which == 0 ? (int)sizeof(lg_dec_member_outcome_buffers) : -1; }

}  // extern "C"
