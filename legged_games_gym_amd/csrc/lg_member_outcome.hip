// lg_member_outcome.hip -- the post stage of the decentralised predator-prey game with the outcome statistics kept per opponent-pool member
// (include/legged_dec_game_member_outcome.h): k_member_outcome, reached through launch_member_outcome.  A translation unit of its own, as
// every game kernel outside lg_game.h is, so that the code hipcc generates for the other kernels does not depend on it (see lg_game.h).
// The C entry point is in lg_member_outcome_entry.h (lg_game_entry.hip).
//
// The per-env body is dec_post_env<true> (lg_dec_game_post.h) and the pooled reductions are those of k_dec_outcome (lg_dec_game_outcome.hip),
// the same functions (lg_outcome_reduce.h), so everything that kernel writes comes out bit-identical.  The addition: a pool block is 32 envs and a wave 64, so
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
#include "lg_outcome_reduce.h"
#include "../../include/legged_dec_game_member_outcome.h"

namespace lg {

#define LG_MO_HALVES (LG_DEC_BLOCK / LG_DEC_POOL_BLOCK_ENVS)                               // pool blocks per workgroup: 8
#define LG_MO_PAIRS (LG_DEC_MEMBER_OUTCOME_ROWS * LG_DEC_OUTCOME_NUM_COUNTS)               // (member, count) pairs: 96
#define LG_MO_CONST_AS __attribute__((address_space(4)))
static_assert(LG_DEC_POOL_BLOCK_ENVS == 32 && LG_DEC_BLOCK % 64 == 0 && LG_MO_PAIRS <= LG_DEC_BLOCK, "a half-wave is one pool block");

// amdgpu_num_sgpr(96): as k_dec_outcome, whose by-value arguments already exceed what 8 waves/SIMD allow; three more pointers here.
// At that cap the last workgroup publishes the episode means inside the counts' branch and in front of them: as a branch of their own, or
// behind the counts, hipcc leaves a private segment of 68 bytes that no instruction uses.

__global__ __launch_bounds__(LG_DEC_BLOCK) __attribute__((amdgpu_num_sgpr(96))) void k_member_outcome(lg_dec_game_params P, lg_dec_game_buffers B, lg_dec_outcome_buffers O, lg_dec_member_outcome_buffers M, int64_t step_arg) {
#pragma clang fp contract(off)
    __shared__ count_t s_cnt[LG_DEC_WAVES][LG_DEC_OUTCOME_NUM_COUNTS];
    __shared__ float s_part[LG_DEC_WAVES][4];
    __shared__ count_t s_half[LG_MO_HALVES][LG_DEC_OUTCOME_NUM_COUNTS];                    // the eight half-wave records: counts ...
    __shared__ int s_slot[LG_MO_HALVES];                                                    // ... and member
    __shared__ int s_last;
    const int e = blockIdx.x * LG_DEC_BLOCK + threadIdx.x;
    float red[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    unsigned flags = 0;
    count_t steps = 0, cnt[LG_DEC_OUTCOME_NUM_COUNTS], hcnt[LG_DEC_OUTCOME_NUM_COUNTS];
    if (e < P.num_envs) flags = dec_post_env<true>(P, B, O.ll_time_out_buf, e, step_arg >= 0 ? step_arg : B.ll_step_counter[0], red, &steps);

    // every lane of the workgroup arrives here: episode sums and pooled counts as in k_dec_outcome, the half's counts from the same ballots
    wave_sum4(red);
    wave_counts(flags, steps, cnt, hcnt);
    store_wave_partials(s_part, red);
    store_wave_partials(s_cnt, cnt);
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
    count_t *maccum = reinterpret_cast<count_t *>(M.member_accum);
    if (threadIdx.x < LG_MO_PAIRS) {
        const int m = threadIdx.x / LG_DEC_OUTCOME_NUM_COUNTS, i = threadIdx.x - m * LG_DEC_OUTCOME_NUM_COUNTS;
        count_t sum = 0;
#pragma unroll
        for (int h = 0; h < LG_MO_HALVES; h++) sum += s_slot[h] == m ? s_half[h][i] : 0ull;
        if (sum != 0) {
            __hip_atomic_fetch_add(maccum + threadIdx.x, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            release_adds();      // performed before this thread passes the barrier behind which thread 0 draws the ticket
        }
    }
    __syncthreads();

    if (threadIdx.x == 0) {      // what k_dec_outcome's thread 0 does, with `last` handed to the workgroup
        float tot[4];
        count_t itot[LG_DEC_OUTCOME_NUM_COUNTS];
        sum_wave_partials(s_part, tot);
        sum_wave_partials(s_cnt, itot);
        if (itot[0] != 0) {
            add_episode_sums(B.extras_accum, tot);
            add_counts(O.accum, itot);
        }
        const bool last = draw_last_ticket(B.extras_ticket);
        if (last) {
            if (load_counts(O.accum, itot)) {                          // itot: now the launch's
                publish_episode_means<false>(B.extras_accum, B.episode_means, P.max_episode_length_s);
                publish_counts(itot, O.accum, O.totals, O.means);
            }
            reset_ticket(B.extras_ticket);
        }
        s_last = last;
    }
    __syncthreads();
    if (!s_last || threadIdx.x >= LG_MO_PAIRS) return;
    // the last workgroup, one pair per thread: every other workgroup's adds were performed before its ticket, which thread 0 has seen
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const count_t v = __hip_atomic_load(maccum + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v != 0) {                                                      // a launch without a done env of this member leaves its totals as they are
        M.member_totals[threadIdx.x] = M.member_totals[threadIdx.x] + v;      // the single writer: launches on one stream
        __hip_atomic_store(maccum + threadIdx.x, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

int launch_member_outcome(const lg_dec_game_params &P, const lg_dec_game_buffers &B, const lg_dec_outcome_buffers &O, const lg_dec_member_outcome_buffers &M, int64_t step, void *stream) {
    hipLaunchKernelGGL(k_member_outcome, dec_grid(P), dim3(LG_DEC_BLOCK), 0, (hipStream_t)stream, P, B, O, M, step);
    return (int)hipGetLastError();
}

}  // namespace lg
