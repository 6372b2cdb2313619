// lg_dec_game.hip -- the kernels of the decentralised predator-prey game (include/legged_dec_game.h): k_dec_pre / k_dec_post, and the
// lg_policy_act instantiations for actors with one input tile (the 16-input prey actor, the 3-input predator actor).  A translation unit of
// its own, reached through the launchers of lg_dec_game_common.h, so that the code hipcc generates for the kernels of lg_kernels.hip does
// not depend on it (see lg_game.h).  The C entry points are in lg_dec_game.h (lg_game_entry.hip).
//
// Floating point: contraction is OFF in k_dec_pre / k_dec_post, every expression rounds once per operation in the order written, so the
// results are bit-comparable with the NumPy float32 restatement (tests/dec_game_twin.py) except behind sqrtf / acosf (1 ulp on this build)
// and in the episode means, whose summation order over workgroups is not fixed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define LG_POLICY_BLOCKS_ONLY      // lg_policy.h without its two non-template pack kernels (they belong to lg_learner.hip)
#include "lg_device.h"
#include "lg_policy.h"
#include "lg_dec_game_post.h"  // dec_post_env<OUTCOME>: one env of the post stage (shared with lg_dec_game_outcome.hip)
#include "lg_outcome_reduce.h" // the reductions, the ticket and the publication behind it (shared with every outcome kernel)
#include "lg_dec_game_common.h"
#include "lg_dec_game_act.h"   // dec_actor_role<ROLE>: one role of the shared actor launch (shared with lg_pool_act.hip)

namespace lg {

__global__ __launch_bounds__(LG_DEC_BLOCK) void k_dec_pre(lg_dec_game_params P, lg_dec_game_buffers B) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * LG_DEC_BLOCK + threadIdx.x;
    if (e >= P.num_envs) return;
    float *c = B.command_prey + (size_t)e * LG_DEC_NUM_ACTIONS_PREY;
    const float c0 = game_clip(c[0], P.cmd_lin_vel_x[0], P.cmd_lin_vel_x[1]);                 // (:182-183)
    const float c1 = game_clip(c[1], P.cmd_lin_vel_y[0], P.cmd_lin_vel_y[1]);
    const float c2 = P.heading_command ? game_wrap_to_pi(c[2]) : c[2];                        // (:185) column 2, as the reference
    const float c3 = c[3];
    c[0] = c0; c[1] = c1; c[2] = c2;
    float *ll = B.ll_commands + (size_t)e * 4;                                                // (:195)
    ll[0] = c0; ll[1] = c1; ll[2] = c2; ll[3] = c3;
    float *d = B.command_pred + (size_t)e * LG_DEC_NUM_ACTIONS_PRED;                          // (:188-189)
    const float d0 = game_clip(d[0], P.predator_lin_vel_x[0], P.predator_lin_vel_x[1]);
    const float d1 = game_clip(d[1], P.predator_lin_vel_y[0], P.predator_lin_vel_y[1]);
    d[0] = d0; d[1] = d1;
}

__global__ __launch_bounds__(LG_DEC_BLOCK) void k_dec_post(lg_dec_game_params P, lg_dec_game_buffers B, int64_t step_arg) {
#pragma clang fp contract(off)
    __shared__ float s_part[LG_DEC_WAVES][4];
    const int e = blockIdx.x * LG_DEC_BLOCK + threadIdx.x;
    float red[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (e < P.num_envs) dec_post_env<false>(P, B, nullptr, e, step_arg >= 0 ? step_arg : B.ll_step_counter[0], red, nullptr);
    // extras["episode"] (:298-305): count and episode sums of this workgroup's done envs -> one atomic per value -> the workgroup with the
    // last ticket publishes the means and leaves accumulator and ticket zeroed for the next launch (lg_outcome_reduce.h)
    wave_sum4(red);
    store_wave_partials(s_part, red);
    __syncthreads();
    if (threadIdx.x != 0) return;
    float tot[4];
    sum_wave_partials(s_part, tot);
    if (tot[0] > 0.0f) add_episode_sums(B.extras_accum, tot);
    if (!draw_last_ticket(B.extras_ticket)) return;
    publish_episode_means<true>(B.extras_accum, B.episode_means, P.max_episode_length_s);
    reset_ticket(B.extras_ticket);
}

int launch_dec_pre(const lg_dec_game_params &P, const lg_dec_game_buffers &B, void *stream) {
    hipLaunchKernelGGL(k_dec_pre, dec_grid(P), dim3(LG_DEC_BLOCK), 0, (hipStream_t)stream, P, B);
    return (int)hipGetLastError();
}

int launch_dec_post(const lg_dec_game_params &P, const lg_dec_game_buffers &B, int64_t step, void *stream) {
    hipLaunchKernelGGL(k_dec_post, dec_grid(P), dim3(LG_DEC_BLOCK), 0, (hipStream_t)stream, P, B, step);
    return (int)hipGetLastError();
}

// the actor kernels are compiled with the default contraction, as in lg_learner.hip: the pragmas above are function-local
int launch_policy_act_one_tile(const PolicyArgs &A, void *stream) {
    hipLaunchKernelGGL((k_policy_act<1, 32, 16, 8>), dim3((A.num_envs + 15) / 16), dim3(64 * LG_POLICY_WAVES), 0, (hipStream_t)stream, A);
    return (int)hipGetLastError();
}

int launch_policy_act_wide_one_tile(const PolicyWideArgs &W, void *stream) {
    hipLaunchKernelGGL((k_policy_act_wide<1, 16, 8, 4>), dim3((W.base.num_envs + LG_PW_ENVS - 1) / LG_PW_ENVS), dim3(64 * LG_PW_WAVES), 0, (hipStream_t)stream, W);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------ k_dec_act (lg_dec_game_act): the roles are dec_actor_role (lg_dec_game_act.h)
__global__ void __launch_bounds__(64 * LG_PW_WAVES) k_dec_act(const DecActArgs G) {
    __shared__ bf16x8g xa[16][2][64], xb[32][2][64];               // as k_policy_act_wide: obs / x2 in xa, x1 / x3 in xb (96 KB), the same for all roles
    const int role = (int)blockIdx.x / G.blocks, blk = (int)blockIdx.x - role * G.blocks;      // every role has `blocks` workgroups, the low-level role the first
    if (role == 0) dec_actor_role<0>(G.ll, G, blk, xa, xb);
    else if (role == 1) dec_actor_role<1>(G.prey, G, blk, xa, xb);
    else dec_actor_role<2>(G.pred, G, blk, xa, xb);
}

int launch_dec_act(const DecActArgs &G, void *stream) {
    hipLaunchKernelGGL(k_dec_act, dim3(3 * G.blocks), dim3(64 * LG_PW_WAVES), 0, (hipStream_t)stream, G);
    return (int)hipGetLastError();
}

}  // namespace lg
