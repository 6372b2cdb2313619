// lg_pursuer_game.h -- C entry points of the scripted pursuer (include/legged_pursuer_game.h).  Host code only: the kernel lives in
// lg_pursuer_game.hip behind launch_pursuer_post.  Included from lg_kernels.hip after its error helpers (fail / HIP_TRY).
#pragma once
#include "../../include/legged_pursuer_game.h"

namespace lg {
int launch_pursuer_post(const lg_game_params &P, const lg_pursuer_params &Q, const lg_game_buffers &B, float *predator_command, int64_t step,
                        void *stream);                                  // lg_pursuer_game.hip; returns the hipError_t of the launch
}

extern "C" {

// the ranges of the scripted rule (Q is not null): game_quotient is exact for 1 <= L <= 2^20
static int pursuer_check(const lg_pursuer_params *Q) {
    if (Q->max_episode_length < 1 || Q->max_episode_length > (1 << 20))
        return fail(-2, "lg_pursuer_params: max_episode_length must be in 1 .. 2^20");
    if (!(Q->max_lin_vel >= Q->min_lin_vel)) return fail(-2, "lg_pursuer_params: max_lin_vel must not be below min_lin_vel");
    if (!(Q->gain > 0.0f)) return fail(-2, "lg_pursuer_params: gain must be positive");
    return 0;
}

int lg_pursuer_post(const lg_game_params *P, const lg_pursuer_params *Q, const lg_game_buffers *B, float *predator_command, int64_t common_step_counter,
                    void *stream) {
    if (!Q) return fail(-1, "null argument");
    if (int rc = game_check(P, B)) return rc;
    if (int rc = pursuer_check(Q)) return rc;
    if (int rc = game_post_check("lg_pursuer_post", B, false, common_step_counter)) return rc;
    HIP_TRY((hipError_t)lg::launch_pursuer_post(*P, *Q, *B, predator_command, common_step_counter, stream));
    return 0;
}

int lg_pursuer_sizeof(int which) { return which == 0 ? (int)sizeof(lg_pursuer_params) : -1; }

}  // extern "C"
