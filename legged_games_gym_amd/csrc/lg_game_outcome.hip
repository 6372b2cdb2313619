// lg_game_outcome.hip -- the post stage of the predator-prey game with outcome statistics (include/legged_game_outcome.h): the two
// instantiations of k_outcome_post (lg_game_outcome.h), reached through launch_outcome_post.  A translation unit of its own, as every game
// kernel outside lg_game.h is, so that the code hipcc generates for the kernels of lg_kernels.hip does not depend on it (see lg_game.h).
// The C entry points are in lg_game_outcome_entry.h (lg_game_entry.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#define LG_POLICY_BLOCKS_ONLY      // lg_policy.h (which lg_game_common.h needs) without its two non-template pack kernels
#include "lg_device.h"
#include "lg_policy.h"
#include "lg_game_outcome.h"

namespace lg {

int launch_outcome_post(bool scripted, const lg_game_params &P, const lg_pursuer_params &Q, const lg_game_buffers &B, const lg_outcome_buffers &O,
                        float *predator_command, int64_t step, void *stream) {
    const dim3 grid((P.num_envs + LG_OUTCOME_BLOCK - 1) / LG_OUTCOME_BLOCK), block(LG_OUTCOME_BLOCK);
    if (scripted) hipLaunchKernelGGL(k_outcome_post<true>, grid, block, 0, (hipStream_t)stream, P, Q, B, O, predator_command, step);
    else hipLaunchKernelGGL(k_outcome_post<false>, grid, block, 0, (hipStream_t)stream, P, Q, B, O, predator_command, step);
    return (int)hipGetLastError();
}

}  // namespace lg
