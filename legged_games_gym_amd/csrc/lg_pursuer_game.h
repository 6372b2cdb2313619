// lg_pursuer_game.h -- C entry points of the scripted pursuer (include/legged_pursuer_game.h).  Host code only: the kernel lives in
// lg_pursuer_game.hip behind launch_pursuer_post.  An entry header of lg_game_entry.hip; includes what it uses.
#pragma once
#include "lg_game.h"                // fail / HIP_TRY (lg_host.h), game_check, game_post_check
#include "../../include/legged_pursuer_game.h"

namespace lg {
int launch_pursuer_post(const lg_game_params &P, const lg_pursuer_params &Q, const lg_game_buffers &B, float *predator_command, int64_t step,
                        void *stream);                                  // lg_pursuer_game.hip; returns the hipError_t of the launch
}

extern "C" {

// the ranges of the scripted rule (Q is not null): game_quotient is exact for 1 <= L <= 2^20
static int pursuer_check(const lg_pursuer_params *Q) {
    if (Q->max_episode_length < 1 || Q->max_episode_length > (1 << 20))
        return lg::fail(-2, "lg_pursuer_params: max_episode_length must be in 1 .. 2^20");
    if (!(Q->max_lin_vel >= Q->min_lin_vel)) return lg::fail(-2, "lg_pursuer_params: max_lin_vel must not be below min_lin_vel");
    if (!(Q->gain > 0.0f)) return lg::fail(-2, "lg_pursuer_params: gain must be positive");
    return 0;
}

int lg_pursuer_post(const lg_game_params *P, const lg_pursuer_params *Q, const lg_game_buffers *B, float *predator_command, int64_t common_step_counter,
                    void *stream) {
    if (!Q) return lg::fail(-1, "null argument");
    if (int rc = game_check(P, B)) return rc;
    if (int rc = pursuer_check(Q)) return rc;
    if (int rc = game_post_check("lg_pursuer_post", B, false, common_step_counter)) return rc;
    HIP_TRY((hipError_t)lg::launch_pursuer_post(*P, *Q, *B, predator_command, common_step_counter, stream));
    return 0;
}

int lg_pursuer_sizeof(int which) { return which == 0 ? (int)sizeof(lg_pursuer_params) : -1; }

}  // extern "C"
