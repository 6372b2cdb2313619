// lg_game_outcome.h -- k_outcome_post<SCRIPTED>: the post stage of the predator-prey game with the outcome statistics of
// include/legged_game_outcome.h.  The per-env body is game_post_env<SCRIPTED, true> (lg_game_post.h), the one k_game_post (SCRIPTED = false)
// and k_pursuer_post (SCRIPTED = true) run, so everything those kernels write comes out bit-identical.  Included from lg_game_outcome.hip only.
//
// The addition: where the plain kernels fold the causes of an episode's end into `done`, this one gets them back as flags, counts them over
// the launch with integers only -- ballot + popcount per wave, LDS per workgroup, one 64-bit agent-scope atomic add per value and workgroup --
// and lets the workgroup that draws the last ticket publish means and totals: the functions of lg_outcome_reduce.h, which k_dec_post runs too.
#pragma once
#include "lg_game_post.h"
#include "lg_outcome_reduce.h"
#include "../../include/legged_game_outcome.h"

namespace lg {

#define LG_OUTCOME_BLOCK 256
#define LG_OUTCOME_WAVES (LG_OUTCOME_BLOCK / 64)

template <bool SCRIPTED>
__global__ __launch_bounds__(LG_OUTCOME_BLOCK) void k_outcome_post(lg_game_params P, lg_pursuer_params Q, lg_game_buffers B, lg_outcome_buffers O,
                                                                  float *predator_command, int64_t step_arg) {
#pragma clang fp contract(off)
    __shared__ count_t s_part[LG_OUTCOME_WAVES][LG_OUTCOME_NUM_COUNTS];
    const int e = blockIdx.x * LG_OUTCOME_BLOCK + threadIdx.x;
    unsigned flags = 0;
    count_t steps = 0;
    if (e < P.num_envs)
        flags = game_post_env<SCRIPTED, true>(P, Q, B, predator_command, O.ll_time_out_buf, e, step_arg >= 0 ? step_arg : B.ll_step_counter[0], &steps);

    // every lane of the workgroup arrives here (no early return above): six counts per wave from ballots, the step sum from a butterfly;
    // thread 0 adds the workgroup's, draws the ticket and publishes when it is the last (lg_outcome_reduce.h)
    count_t cnt[LG_OUTCOME_NUM_COUNTS], tot[LG_OUTCOME_NUM_COUNTS];
    wave_counts(flags, steps, cnt);
    store_wave_partials(s_part, cnt);
    __syncthreads();
    if (threadIdx.x != 0) return;
    sum_wave_partials(s_part, tot);
    if (tot[0] != 0) add_counts(O.accum, tot);
    if (!draw_last_ticket(O.ticket)) return;
    if (load_counts(O.accum, tot)) publish_counts(tot, O.accum, O.totals, O.means);      // tot: now the launch's
    reset_ticket(O.ticket);
}

}  // namespace lg
