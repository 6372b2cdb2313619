// lg_pursuer_game.h -- C entry points of the scripted pursuer (include/legged_pursuer_game.h).  Host code only: the kernel lives in
// lg_pursuer_game.hip behind launch_pursuer_post.  Included from lg_kernels.hip after its error helpers (fail / HIP_TRY).
#pragma once
#include "../../include/legged_pursuer_game.h"

namespace lg {
int launch_pursuer_post(const lg_game_params &P, const lg_pursuer_params &Q, const lg_game_buffers &B, float *predator_command, int64_t step,
                        void *stream);                                  // lg_pursuer_game.hip; returns the hipError_t of the launch
}

extern "C" {

int lg_pursuer_post(const lg_game_params *P, const lg_pursuer_params *Q, const lg_game_buffers *B, float *predator_command, int64_t common_step_counter,
                    void *stream) {
    if (!Q) return fail(-1, "null argument");
    if (int rc = game_check(P, B)) return rc;
    if (Q->max_episode_length < 1 || Q->max_episode_length > (1 << 20))
        return fail(-2, "lg_pursuer_params: max_episode_length must be in 1 .. 2^20");
    if (!(Q->max_lin_vel >= Q->min_lin_vel)) return fail(-2, "lg_pursuer_params: max_lin_vel must not be below min_lin_vel");
    if (!(Q->gain > 0.0f)) return fail(-2, "lg_pursuer_params: gain must be positive");
    if (!B->ll_root_states || !B->ll_env_origins || !B->ll_rew_buf || !B->ll_reset_buf || !B->predator_pos || !B->obs || !B->rew || !B->reset_buf ||
        !B->curr_episode_step || !B->episode_length_buf || !B->episode_sums) return fail(-1, "lg_pursuer_post: a buffer pointer is null");
    if (common_step_counter < 0 && !B->ll_step_counter) return fail(-9, "common_step_counter = -1 needs the low-level step_counter buffer");
    HIP_TRY((hipError_t)lg::launch_pursuer_post(*P, *Q, *B, predator_command, common_step_counter, stream));
    return 0;
}

int lg_pursuer_sizeof(int which) { return which == 0 ? (int)sizeof(lg_pursuer_params) : -1; }

}  // extern "C"
