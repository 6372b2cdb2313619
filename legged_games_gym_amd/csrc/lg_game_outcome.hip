// lg_game_outcome.hip -- the post stage of the predator-prey game with outcome statistics (include/legged_game_outcome.h): the two
// instantiations of k_outcome_post (lg_game_outcome.h) and their C entry points.  A translation unit of its own that nothing else includes
// or calls into, so that the code hipcc generates for every other kernel of the library does not depend on it (see lg_game.h).
//
// Floating point: contraction is OFF in the kernel, as in k_game_post / k_pursuer_post, whose outputs it reproduces bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#define LG_POLICY_BLOCKS_ONLY      // lg_policy.h (which lg_game_common.h needs) without its two non-template pack kernels
#include "lg_device.h"
#include "lg_policy.h"
#include "lg_game_outcome.h"
#include "../../include/legged_hip.h"

// The error text of the library is a thread-local buffer of lg_kernels.hip (512 bytes) that lg_last_error() hands out; the entry points
// here leave their message in it through that pointer, so callers read it where they read every other one.
static int outcome_fail(int code, const char *fmt, const char *arg = "") {
    snprintf(const_cast<char *>(lg_last_error()), 256, fmt, arg);
    return code;
}
#define OUTCOME_HIP_TRY(x) do { hipError_t _e = (x); if (_e != hipSuccess) return outcome_fail(-10, "HIP error: %s", hipGetErrorString(_e)); } while (0)

// the checks of lg_game_post (lg_game.h), then those of the outcome buffers
static int outcome_check(const char *who, const lg_game_params *P, const lg_game_buffers *B, const lg_outcome_buffers *O, bool need_command,
                         int64_t common_step_counter) {
    if (!P || !B || !O) return outcome_fail(-1, "null argument");
    if (P->num_envs < 1 || P->decimation < 0) return outcome_fail(-2, "lg_game_params: num_envs must be >= 1 and decimation >= 0");
    if ((need_command && !B->command) || !B->ll_root_states || !B->ll_env_origins || !B->ll_rew_buf || !B->ll_reset_buf || !B->predator_pos || !B->obs ||
        !B->rew || !B->reset_buf || !B->curr_episode_step || !B->episode_length_buf || !B->episode_sums)
        return outcome_fail(-1, "%s: a buffer pointer is null", who);
    if (!O->ll_time_out_buf || !O->accum || !O->ticket || !O->means || !O->totals) return outcome_fail(-1, "%s: a pointer of lg_outcome_buffers is null", who);
    if (common_step_counter < 0 && !B->ll_step_counter) return outcome_fail(-9, "common_step_counter = -1 needs the low-level step_counter buffer");
    return 0;
}

extern "C" {

int lg_outcome_post(const lg_game_params *P, const lg_game_buffers *B, const lg_outcome_buffers *O, int64_t common_step_counter, void *stream) {
    if (int rc = outcome_check("lg_outcome_post", P, B, O, true, common_step_counter)) return rc;
    const lg_pursuer_params none = {0.0f, 0.0f, 0.0f, 0};
    hipLaunchKernelGGL(lg::k_outcome_post<false>, dim3((P->num_envs + LG_OUTCOME_BLOCK - 1) / LG_OUTCOME_BLOCK), dim3(LG_OUTCOME_BLOCK), 0,
                       (hipStream_t)stream, *P, none, *B, *O, (float *)nullptr, common_step_counter);
    OUTCOME_HIP_TRY(hipGetLastError());
    return 0;
}

int lg_outcome_pursuer_post(const lg_game_params *P, const lg_pursuer_params *Q, const lg_game_buffers *B, const lg_outcome_buffers *O,
                            float *predator_command, int64_t common_step_counter, void *stream) {
    if (!Q) return outcome_fail(-1, "null argument");
    if (!P || !B || !O) return outcome_fail(-1, "null argument");
    if (P->num_envs < 1 || P->decimation < 0) return outcome_fail(-2, "lg_game_params: num_envs must be >= 1 and decimation >= 0");
    if (Q->max_episode_length < 1 || Q->max_episode_length > (1 << 20))
        return outcome_fail(-2, "lg_pursuer_params: max_episode_length must be in 1 .. 2^20");
    if (!(Q->max_lin_vel >= Q->min_lin_vel)) return outcome_fail(-2, "lg_pursuer_params: max_lin_vel must not be below min_lin_vel");
    if (!(Q->gain > 0.0f)) return outcome_fail(-2, "lg_pursuer_params: gain must be positive");
    if (int rc = outcome_check("lg_outcome_pursuer_post", P, B, O, false, common_step_counter)) return rc;
    hipLaunchKernelGGL(lg::k_outcome_post<true>, dim3((P->num_envs + LG_OUTCOME_BLOCK - 1) / LG_OUTCOME_BLOCK), dim3(LG_OUTCOME_BLOCK), 0,
                       (hipStream_t)stream, *P, *Q, *B, *O, predator_command, common_step_counter);
    OUTCOME_HIP_TRY(hipGetLastError());
    return 0;
}

int lg_outcome_sizeof(int which) { return which == 0 ? (int)sizeof(lg_outcome_buffers) : -1; }

}  // extern "C"
