// lg_dec_game_outcome.hip -- the post stage of the decentralised predator-prey game with outcome statistics
// (include/legged_dec_game_outcome.h): k_dec_outcome, reached through launch_dec_outcome.  A translation unit of its own, as every game
// kernel outside lg_game.h is, so that the code hipcc generates for the kernels of lg_kernels.hip and lg_dec_game.hip does not depend on
// it (see lg_game.h).  The C entry point is in lg_dec_game_outcome_entry.h (lg_game_entry.hip).
//
// The per-env body is dec_post_env<true> (lg_dec_game_post.h), the one k_dec_post runs with OUTCOME = false, so everything that kernel
// writes per env comes out bit-identical.  The addition: where k_dec_post folds the causes of an episode's end into `done`, this kernel
// gets them back as flags, counts them over the launch with integers only -- ballot + popcount per wave, LDS per workgroup, one 64-bit
// agent-scope atomic add per non-zero value and workgroup -- next to the float episode sums of k_dec_post, and lets the workgroup that
// draws the last ticket publish both.  ONE ticket per workgroup and launch (extras_ticket) serves both reductions.  Reductions, ticket and
// publication are the functions of lg_outcome_reduce.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define LG_POLICY_BLOCKS_ONLY      // lg_policy.h (which lg_game_common.h needs) without its two non-template pack kernels
#include "lg_device.h"
#include "lg_policy.h"
#include "lg_dec_game_post.h"
#include "lg_outcome_reduce.h"
#include "../../include/legged_dec_game_outcome.h"

namespace lg {

// amdgpu_num_sgpr(96): k_dec_post holds 94 scalar registers (parameters and 22 pointers by value); the four pointers of
// lg_dec_outcome_buffers made it 102 here, over the 96 that 8 waves/SIMD allow.  Under the cap hipcc fetches them later: 94, nothing spilled.

__global__ __launch_bounds__(LG_DEC_BLOCK) __attribute__((amdgpu_num_sgpr(96))) void k_dec_outcome(lg_dec_game_params P, lg_dec_game_buffers B, lg_dec_outcome_buffers O, int64_t step_arg) {
#pragma clang fp contract(off)
    __shared__ count_t s_cnt[LG_DEC_WAVES][LG_DEC_OUTCOME_NUM_COUNTS];
    __shared__ float s_part[LG_DEC_WAVES][4];
    const int e = blockIdx.x * LG_DEC_BLOCK + threadIdx.x;
    float red[4] = {0.0f, 0.0f, 0.0f, 0.0f}, tot[4];
    unsigned flags = 0;
    count_t steps = 0, cnt[LG_DEC_OUTCOME_NUM_COUNTS], itot[LG_DEC_OUTCOME_NUM_COUNTS];
    if (e < P.num_envs) flags = dec_post_env<true>(P, B, O.ll_time_out_buf, e, step_arg >= 0 ? step_arg : B.ll_step_counter[0], red, &steps);

    // every lane of the workgroup arrives here.  The float episode sums exactly as k_dec_post reduces them; five counts per wave from
    // ballots, the step sum from a butterfly; thread 0 adds both, draws the one ticket and publishes both when it is the last
    wave_sum4(red);
    wave_counts(flags, steps, cnt);
    store_wave_partials(s_part, red);
    store_wave_partials(s_cnt, cnt);
    __syncthreads();
    if (threadIdx.x != 0) return;
    sum_wave_partials(s_part, tot);
    sum_wave_partials(s_cnt, itot);
    if (itot[0] != 0) {                                            // (= tot[0] > 0: both count this workgroup's done envs)
        add_episode_sums(B.extras_accum, tot);
        add_counts(O.accum, itot);
    }
    if (!draw_last_ticket(B.extras_ticket)) return;
    if (load_counts(O.accum, itot)) {                              // itot: now the launch's
        publish_episode_means<false>(B.extras_accum, B.episode_means, P.max_episode_length_s);
        publish_counts(itot, O.accum, O.totals, O.means);
    }
    reset_ticket(B.extras_ticket);
}

int launch_dec_outcome(const lg_dec_game_params &P, const lg_dec_game_buffers &B, const lg_dec_outcome_buffers &O, int64_t step, void *stream) {
    hipLaunchKernelGGL(k_dec_outcome, dec_grid(P), dim3(LG_DEC_BLOCK), 0, (hipStream_t)stream, P, B, O, step);
    return (int)hipGetLastError();
}

}  // namespace lg
