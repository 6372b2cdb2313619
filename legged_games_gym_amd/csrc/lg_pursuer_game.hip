// lg_pursuer_game.hip -- k_pursuer_post: the post stage of the predator-prey game with the reference's scripted pursuer
// (include/legged_pursuer_game.h; reference high_level_game.py:265-324 with `command=None`).  A translation unit of its own, reached through
// launch_pursuer_post, so that the code hipcc generates for the kernels of lg_kernels.hip does not depend on it (see lg_game.h).  The C
// entry points are in lg_pursuer_game.h (lg_game_entry.hip).
//
// The body is game_post_env<true, false> (lg_game_post.h), shared with the other post kernels: k_game_post with the predator's velocity
// computed by the scripted rule in place of the two loads from `command`.  Floating point: contraction is OFF there, so the results are
// bit-comparable with the NumPy float32 restatement (tests/pursuer_twin.py) except behind sqrtf / acosf (1 ulp on this build).
#include <hip/hip_runtime.h>
#include <stdint.h>

#define LG_POLICY_BLOCKS_ONLY      // lg_policy.h (which lg_game_common.h needs) without its two non-template pack kernels
#include "lg_device.h"
#include "lg_policy.h"
#include "lg_game_post.h"

namespace lg {

#define LG_PURSUER_BLOCK 256

__global__ __launch_bounds__(LG_PURSUER_BLOCK) void k_pursuer_post(lg_game_params P, lg_pursuer_params Q, lg_game_buffers B, float *predator_command,
                                                                  int64_t step_arg) {
    const int e = blockIdx.x * LG_PURSUER_BLOCK + threadIdx.x;
    if (e >= P.num_envs) return;
    game_post_env<true, false>(P, Q, B, predator_command, nullptr, e, step_arg >= 0 ? step_arg : B.ll_step_counter[0], nullptr);
}

int launch_pursuer_post(const lg_game_params &P, const lg_pursuer_params &Q, const lg_game_buffers &B, float *predator_command, int64_t step,
                        void *stream) {
    hipLaunchKernelGGL(k_pursuer_post, dim3((P.num_envs + LG_PURSUER_BLOCK - 1) / LG_PURSUER_BLOCK), dim3(LG_PURSUER_BLOCK), 0, (hipStream_t)stream,
                       P, Q, B, predator_command, step);
    return (int)hipGetLastError();
}

}  // namespace lg
