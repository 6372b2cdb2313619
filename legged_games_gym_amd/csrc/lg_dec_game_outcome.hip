// lg_dec_game_outcome.hip -- the post stage of the decentralised predator-prey game with outcome statistics
// (include/legged_dec_game_outcome.h): k_dec_outcome, reached through launch_dec_outcome.  A translation unit of its own, as every game
// kernel outside lg_game.h is, so that the code hipcc generates for the kernels of lg_kernels.hip and lg_dec_game.hip does not depend on
// it (see lg_game.h).  The C entry point is in lg_dec_game_outcome_entry.h (lg_kernels.hip).
//
// The per-env body is dec_post_env<true> (lg_dec_game_post.h), the one k_dec_post runs with OUTCOME = false, so everything that kernel
// writes per env comes out bit-identical.  The addition: where k_dec_post folds the causes of an episode's end into `done`, this kernel
// gets them back as flags, counts them over the launch with integers only -- ballot + popcount per wave, LDS per workgroup, one 64-bit
// agent-scope atomic add per non-zero value and workgroup -- next to the float episode sums of k_dec_post, and lets the workgroup that
// draws the last ticket publish both.  ONE ticket per workgroup and launch (extras_ticket) serves both reductions.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define LG_POLICY_BLOCKS_ONLY      // lg_policy.h (which lg_game_common.h needs) without its two non-template pack kernels
#include "lg_device.h"
#include "lg_policy.h"
#include "lg_dec_game_post.h"
#include "../../include/legged_dec_game_outcome.h"

namespace lg {

#define LG_DEC_WAVES (LG_DEC_BLOCK / 64)

// amdgpu_num_sgpr(96): k_dec_post holds 94 scalar registers (parameters and 22 pointers by value); the four pointers of
// lg_dec_outcome_buffers made it 102 here, over the 96 that 8 waves/SIMD allow.  Under the cap hipcc fetches them later: 94, nothing spilled.

__global__ __launch_bounds__(LG_DEC_BLOCK) __attribute__((amdgpu_num_sgpr(96))) void k_dec_outcome(lg_dec_game_params P, lg_dec_game_buffers B, lg_dec_outcome_buffers O, int64_t step_arg) {
#pragma clang fp contract(off)
    __shared__ unsigned long long s_cnt[LG_DEC_WAVES][LG_DEC_OUTCOME_NUM_COUNTS];
    __shared__ float s_part[LG_DEC_WAVES][4];
    const int e = blockIdx.x * LG_DEC_BLOCK + threadIdx.x;
    float red[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    unsigned flags = 0;
    unsigned long long steps = 0;
    if (e < P.num_envs) flags = dec_post_env<true>(P, B, O.ll_time_out_buf, e, step_arg >= 0 ? step_arg : B.ll_step_counter[0], red, &steps);

    // every lane of the workgroup arrives here.  The float episode sums exactly as k_dec_post reduces them; five counts per wave from
    // ballots, the step sum from a butterfly
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) red[i] += __shfl_xor(red[i], o);
    unsigned long long cnt[LG_DEC_OUTCOME_NUM_COUNTS];
#pragma unroll
    for (int i = 0; i < 5; i++) cnt[i] = (unsigned long long)__popcll(__ballot((flags >> i) & 1u));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) steps += __shfl_xor(steps, o);
    cnt[5] = steps;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < 4; i++) s_part[threadIdx.x >> 6][i] = red[i];
#pragma unroll
        for (int i = 0; i < LG_DEC_OUTCOME_NUM_COUNTS; i++) s_cnt[threadIdx.x >> 6][i] = cnt[i];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    float tot[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { tot[i] = s_part[0][i]; for (int w = 1; w < LG_DEC_WAVES; w++) tot[i] += s_part[w][i]; }
    unsigned long long itot[LG_DEC_OUTCOME_NUM_COUNTS];
#pragma unroll
    for (int i = 0; i < LG_DEC_OUTCOME_NUM_COUNTS; i++) { itot[i] = s_cnt[0][i]; for (int w = 1; w < LG_DEC_WAVES; w++) itot[i] += s_cnt[w][i]; }
    unsigned long long *accum = reinterpret_cast<unsigned long long *>(O.accum), *totals = reinterpret_cast<unsigned long long *>(O.totals);
    if (itot[0] != 0) {                                            // (= tot[0] > 0: both count this workgroup's done envs)
#pragma unroll
        for (int i = 0; i < 4; i++) atomicAdd(B.extras_accum + i, tot[i]);
#pragma unroll
        for (int i = 0; i < LG_DEC_OUTCOME_NUM_COUNTS; i++)
            if (i == 0 || itot[i] != 0) __hip_atomic_fetch_add(accum + i, itot[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // this workgroup's adds are performed before its ticket is seen: agent-scope release, and the wait spelled out behind it (the fence's own
    // wait is not relied upon)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned int ticket = __hip_atomic_fetch_add(B.extras_ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ticket != gridDim.x - 1) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    // the last workgroup: the accumulators were updated by other workgroups' atomics, read them past the L1 with agent-scope loads
    unsigned long long v[LG_DEC_OUTCOME_NUM_COUNTS];
#pragma unroll
    for (int i = 0; i < LG_DEC_OUTCOME_NUM_COUNTS; i++) v[i] = __hip_atomic_load(accum + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v[0] != 0) {                                               // a step without a done env leaves every mean and the totals as they are
        const float cnt_f = __hip_atomic_load(B.extras_accum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int i = 0; i < LG_DEC_NUM_SUMS; i++) {
            const float s = __hip_atomic_load(B.extras_accum + 1 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            B.episode_means[i] = s / cnt_f / P.max_episode_length_s;
        }
        const float n = (float)v[0];
#pragma unroll
        for (int i = 0; i < LG_DEC_OUTCOME_NUM_MEANS; i++) O.means[i] = (float)v[i + 1] / n;
#pragma unroll
        for (int i = 0; i < LG_DEC_OUTCOME_NUM_COUNTS; i++) totals[i] = totals[i] + v[i];      // the single writer: launches on one stream
#pragma unroll
        for (int i = 0; i < 4; i++) __hip_atomic_store(B.extras_accum + i, 0.0f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int i = 0; i < LG_DEC_OUTCOME_NUM_COUNTS; i++) __hip_atomic_store(accum + i, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __hip_atomic_store(B.extras_ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

int launch_dec_outcome(const lg_dec_game_params &P, const lg_dec_game_buffers &B, const lg_dec_outcome_buffers &O, int64_t step, void *stream) {
    hipLaunchKernelGGL(k_dec_outcome, dim3((P.num_envs + LG_DEC_BLOCK - 1) / LG_DEC_BLOCK), dim3(LG_DEC_BLOCK), 0, (hipStream_t)stream, P, B, O, step);
    return (int)hipGetLastError();
}

}  // namespace lg
