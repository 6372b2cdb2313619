// lg_game_outcome.h -- k_outcome_post<SCRIPTED>: the post stage of the predator-prey game with the outcome statistics of
// include/legged_game_outcome.h.  The per-env body is game_post_env<SCRIPTED, true> (lg_game_post.h), the one k_game_post (SCRIPTED = false)
// and k_pursuer_post (SCRIPTED = true) run, so everything those kernels write comes out bit-identical.  Included from lg_game_outcome.hip only.
//
// The addition: where the plain kernels fold the causes of an episode's end into `done`, this one gets them back as flags, counts them over
// the launch with integers only -- ballot + popcount per wave, LDS per workgroup, one 64-bit agent-scope atomic add per value and workgroup --
// and lets the workgroup that draws the last ticket publish means and totals (the scheme of k_dec_post, lg_dec_game.hip).
#pragma once
#include "lg_game_post.h"
#include "../../include/legged_game_outcome.h"

namespace lg {

#define LG_OUTCOME_BLOCK 256
#define LG_OUTCOME_WAVES (LG_OUTCOME_BLOCK / 64)

template <bool SCRIPTED>
__global__ __launch_bounds__(LG_OUTCOME_BLOCK) void k_outcome_post(lg_game_params P, lg_pursuer_params Q, lg_game_buffers B, lg_outcome_buffers O,
                                                                  float *predator_command, int64_t step_arg) {
#pragma clang fp contract(off)
    __shared__ unsigned long long s_part[LG_OUTCOME_WAVES][LG_OUTCOME_NUM_COUNTS];
    const int e = blockIdx.x * LG_OUTCOME_BLOCK + threadIdx.x;
    unsigned flags = 0;
    unsigned long long steps = 0;
    if (e < P.num_envs)
        flags = game_post_env<SCRIPTED, true>(P, Q, B, predator_command, O.ll_time_out_buf, e, step_arg >= 0 ? step_arg : B.ll_step_counter[0], &steps);

    // every lane of the workgroup arrives here (no early return above): six counts per wave from ballots, the step sum from a butterfly
    unsigned long long cnt[LG_OUTCOME_NUM_COUNTS];
#pragma unroll
    for (int i = 0; i < 6; i++) cnt[i] = (unsigned long long)__popcll(__ballot((flags >> i) & 1u));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) steps += __shfl_xor(steps, o);
    cnt[6] = steps;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < LG_OUTCOME_NUM_COUNTS; i++) s_part[threadIdx.x >> 6][i] = cnt[i];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    unsigned long long tot[LG_OUTCOME_NUM_COUNTS];
#pragma unroll
    for (int i = 0; i < LG_OUTCOME_NUM_COUNTS; i++) { tot[i] = s_part[0][i]; for (int w = 1; w < LG_OUTCOME_WAVES; w++) tot[i] += s_part[w][i]; }
    unsigned long long *accum = reinterpret_cast<unsigned long long *>(O.accum), *totals = reinterpret_cast<unsigned long long *>(O.totals);
    if (tot[0] != 0) {
#pragma unroll
        for (int i = 0; i < LG_OUTCOME_NUM_COUNTS; i++)
            if (i == 0 || tot[i] != 0) __hip_atomic_fetch_add(accum + i, tot[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // this workgroup's adds are performed before its ticket is seen: agent-scope release, and the wait spelled out behind it (the fence's own
    // wait is not relied upon)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned int ticket = __hip_atomic_fetch_add(O.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ticket != gridDim.x - 1) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    // the last workgroup: the accumulators were updated by other workgroups' atomics, read them past the L1 with agent-scope loads
    unsigned long long v[LG_OUTCOME_NUM_COUNTS];
#pragma unroll
    for (int i = 0; i < LG_OUTCOME_NUM_COUNTS; i++) v[i] = __hip_atomic_load(accum + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v[0] != 0) {                                               // a step without a done env leaves means and totals as they are
        const float n = (float)v[0];
#pragma unroll
        for (int i = 0; i < LG_OUTCOME_NUM_MEANS; i++) O.means[i] = (float)v[i + 1] / n;
#pragma unroll
        for (int i = 0; i < LG_OUTCOME_NUM_COUNTS; i++) totals[i] = totals[i] + v[i];          // the single writer: launches on one stream
#pragma unroll
        for (int i = 0; i < LG_OUTCOME_NUM_COUNTS; i++) __hip_atomic_store(accum + i, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __hip_atomic_store(O.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace lg
