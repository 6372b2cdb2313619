// lg_member_outcome.hip -- the post stage of the decentralised predator-prey game with the outcome statistics kept per opponent-pool member
// (include/legged_dec_game_member_outcome.h): k_member_outcome, reached through launch_member_outcome.  A translation unit of its own, as
// every game kernel outside lg_game.h is, so that the code hipcc generates for the other kernels does not depend on it (see lg_game.h).
// The C entry point is in lg_member_outcome_entry.h (lg_kernels.hip).
//
// The per-env body is dec_post_env<true> (lg_dec_game_post.h) and the pooled reductions are those of k_dec_outcome (lg_dec_game_outcome.hip),
// operation for operation, so everything that kernel writes comes out bit-identical.  The addition: a pool block is 32 envs and a wave 64, so
// every HALF of a wave meets one pool member.  The six counts are also taken per half -- the ballots of k_dec_outcome masked to the half, the
// step sum after five of the butterfly's six steps -- and recorded in LDS with the half's member; 96 threads then each own one (member, count)
// pair, sum the records of that member and issue at most one 64-bit agent-scope atomic add.  Integers only: no count depends on the order of
// arrival.  The ONE ticket of the launch serves this reduction too: in the workgroup that draws the last one, the same 96 threads add
// member_accum into member_totals and zero it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define LG_POLICY_BLOCKS_ONLY      // lg_policy.h (which lg_game_common.h needs) without its two non-template pack kernels
#include "lg_device.h"
#include "lg_policy.h"
#include "lg_dec_game_post.h"
#include "../../include/legged_dec_game_member_outcome.h"

namespace lg {

#define LG_MO_WAVES (LG_DEC_BLOCK / 64)
#define LG_MO_HALVES (LG_DEC_BLOCK / LG_DEC_POOL_BLOCK_ENVS)                               // pool blocks per workgroup: 8
#define LG_MO_PAIRS (LG_DEC_MEMBER_OUTCOME_ROWS * LG_DEC_OUTCOME_NUM_COUNTS)               // (member, count) pairs: 96
#define LG_MO_CONST_AS __attribute__((address_space(4)))
static_assert(LG_DEC_POOL_BLOCK_ENVS == 32 && LG_DEC_BLOCK % 64 == 0 && LG_MO_PAIRS <= LG_DEC_BLOCK, "a half-wave is one pool block");

// amdgpu_num_sgpr(96): as k_dec_outcome, whose by-value arguments already exceed what 8 waves/SIMD allow; three more pointers here.

__global__ __launch_bounds__(LG_DEC_BLOCK) __attribute__((amdgpu_num_sgpr(96))) void k_member_outcome(lg_dec_game_params P, lg_dec_game_buffers B, lg_dec_outcome_buffers O, lg_dec_member_outcome_buffers M, int64_t step_arg) {
#pragma clang fp contract(off)
    __shared__ unsigned long long s_cnt[LG_MO_WAVES][LG_DEC_OUTCOME_NUM_COUNTS];
    __shared__ float s_part[LG_MO_WAVES][4];
    __shared__ unsigned long long s_half[LG_MO_HALVES][LG_DEC_OUTCOME_NUM_COUNTS];         // the eight half-wave records: counts ...
    __shared__ int s_slot[LG_MO_HALVES];                                                    // ... and member
    __shared__ int s_last;
    const int e = blockIdx.x * LG_DEC_BLOCK + threadIdx.x;
    float red[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    unsigned flags = 0;
    unsigned long long steps = 0;
    if (e < P.num_envs) flags = dec_post_env<true>(P, B, O.ll_time_out_buf, e, step_arg >= 0 ? step_arg : B.ll_step_counter[0], red, &steps);

    // every lane of the workgroup arrives here.  The float episode sums and the pooled counts exactly as k_dec_outcome reduces them; the
    // half's counts from the same ballots
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) red[i] += __shfl_xor(red[i], o);
    const unsigned long long half_mask = (threadIdx.x & 32) ? 0xFFFFFFFF00000000ull : 0x00000000FFFFFFFFull;
    unsigned long long cnt[LG_DEC_OUTCOME_NUM_COUNTS], hcnt[LG_DEC_OUTCOME_NUM_COUNTS];
#pragma unroll
    for (int i = 0; i < 5; i++) {
        const unsigned long long b = __ballot((flags >> i) & 1u);
        cnt[i] = (unsigned long long)__popcll(b);
        hcnt[i] = (unsigned long long)__popcll(b & half_mask);
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) steps += __shfl_xor(steps, o);
    hcnt[5] = steps;
    cnt[5] = steps + __shfl_xor(steps, 32);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < 4; i++) s_part[threadIdx.x >> 6][i] = red[i];
#pragma unroll
        for (int i = 0; i < LG_DEC_OUTCOME_NUM_COUNTS; i++) s_cnt[threadIdx.x >> 6][i] = cnt[i];
    }
    if ((threadIdx.x & 31) == 0) {
        // the half's member: the entry of the slot table k_pool_act reads for this block, clamped as there.  The table is not written while
        // the kernel runs: read through the constant address space.  A half past the last block holds no env and counts nothing; its index is
        // kept inside the table.
        const int half = threadIdx.x >> 5, blocks = (P.num_envs + LG_DEC_POOL_BLOCK_ENVS - 1) / LG_DEC_POOL_BLOCK_ENVS;
        const int blk = min((int)blockIdx.x * LG_MO_HALVES + half, blocks - 1);
        s_slot[half] = min(max(((const LG_MO_CONST_AS int32_t *)M.block_slot)[blk], 0), M.count - 1);
#pragma unroll
        for (int i = 0; i < LG_DEC_OUTCOME_NUM_COUNTS; i++) s_half[half][i] = hcnt[i];
    }
    __syncthreads();

    // by member: thread t owns pair (t / 6, t % 6)
    unsigned long long *maccum = reinterpret_cast<unsigned long long *>(M.member_accum), *mtotals = reinterpret_cast<unsigned long long *>(M.member_totals);
    if (threadIdx.x < LG_MO_PAIRS) {
        const int m = threadIdx.x / LG_DEC_OUTCOME_NUM_COUNTS, i = threadIdx.x - m * LG_DEC_OUTCOME_NUM_COUNTS;
        unsigned long long sum = 0;
#pragma unroll
        for (int h = 0; h < LG_MO_HALVES; h++) sum += s_slot[h] == m ? s_half[h][i] : 0ull;
        if (sum != 0) {
            __hip_atomic_fetch_add(maccum + threadIdx.x, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // performed before this thread passes the barrier behind which thread 0 draws the ticket (release and wait as below)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();

    if (threadIdx.x == 0) {
        float tot[4];
#pragma unroll
        for (int i = 0; i < 4; i++) { tot[i] = s_part[0][i]; for (int w = 1; w < LG_MO_WAVES; w++) tot[i] += s_part[w][i]; }
        unsigned long long itot[LG_DEC_OUTCOME_NUM_COUNTS];
#pragma unroll
        for (int i = 0; i < LG_DEC_OUTCOME_NUM_COUNTS; i++) { itot[i] = s_cnt[0][i]; for (int w = 1; w < LG_MO_WAVES; w++) itot[i] += s_cnt[w][i]; }
        unsigned long long *accum = reinterpret_cast<unsigned long long *>(O.accum), *totals = reinterpret_cast<unsigned long long *>(O.totals);
        if (itot[0] != 0) {
#pragma unroll
            for (int i = 0; i < 4; i++) atomicAdd(B.extras_accum + i, tot[i]);
#pragma unroll
            for (int i = 0; i < LG_DEC_OUTCOME_NUM_COUNTS; i++)
                if (i == 0 || itot[i] != 0) __hip_atomic_fetch_add(accum + i, itot[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // this workgroup's adds are performed before its ticket is seen: agent-scope release, and the wait spelled out behind it
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned int ticket = __hip_atomic_fetch_add(B.extras_ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = ticket == gridDim.x - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            // the last workgroup: the accumulators were updated by other workgroups' atomics, read them past the L1 with agent-scope loads
            unsigned long long v[LG_DEC_OUTCOME_NUM_COUNTS];
#pragma unroll
            for (int i = 0; i < LG_DEC_OUTCOME_NUM_COUNTS; i++) v[i] = __hip_atomic_load(accum + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (v[0] != 0) {                                           // a step without a done env leaves every mean and the totals as they are
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
        s_last = last;
    }
    __syncthreads();
    if (!s_last || threadIdx.x >= LG_MO_PAIRS) return;
    // the last workgroup, one pair per thread: every other workgroup's adds were performed before its ticket, which thread 0 has seen
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const unsigned long long v = __hip_atomic_load(maccum + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v != 0) {                                                      // a launch without a done env of this member leaves its totals as they are
        mtotals[threadIdx.x] = mtotals[threadIdx.x] + v;              // the single writer: launches on one stream
        __hip_atomic_store(maccum + threadIdx.x, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

int launch_member_outcome(const lg_dec_game_params &P, const lg_dec_game_buffers &B, const lg_dec_outcome_buffers &O, const lg_dec_member_outcome_buffers &M, int64_t step, void *stream) {
    hipLaunchKernelGGL(k_member_outcome, dim3((P.num_envs + LG_DEC_BLOCK - 1) / LG_DEC_BLOCK), dim3(LG_DEC_BLOCK), 0, (hipStream_t)stream, P, B, O, M, step);
    return (int)hipGetLastError();
}

}  // namespace lg
