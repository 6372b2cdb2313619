// lg_outcome_reduce.h -- the tail of the predator-prey post kernels, each operation written once: k_dec_post, k_outcome_post,
// k_dec_outcome and k_member_outcome are their per-env body followed by these functions.  Device code only; needs lg_device.h.
//
// Every wave reduces its lanes, the wave leaders store to LDS, and behind a barrier thread 0 sums the waves in order 0, 1, 2, ... and adds
// the workgroup's values to a global accumulator with agent-scope atomics -- only when the workgroup had a done env.  It RELEASES, draws a
// TICKET, and the workgroup that draws the last one ACQUIRES, reads the accumulator past the L1 with agent-scope loads, publishes, and leaves
// accumulator and ticket zero for the next launch (launches are on one stream: it is the single writer of what it publishes).  Integer
// counts do not depend on the order in which workgroups arrive; the float sums do, beyond two workgroups.
#pragma once

namespace lg {

typedef unsigned long long count_t;      // uint64_t of the C headers, as the 64-bit atomics and shuffles spell it

// ---------------------------------------------------------------- per wave
LG_DEV void wave_sum4(float (&red)[4]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) red[i] += __shfl_xor(red[i], o);
}

// cnt[i < N-1] = lanes of the wave with bit i of `flags` set, cnt[N-1] = sum of `steps`; hcnt the same over this lane's HALF of the wave
// (k_member_outcome; elsewhere unused and dropped by the compiler).  Integers: cnt is what a butterfly from 32 down gives.
template <int N>
LG_DEV void wave_counts(const unsigned flags, count_t steps, count_t (&cnt)[N], count_t (&hcnt)[N]) {
    const count_t half_mask = (threadIdx.x & 32) ? 0xFFFFFFFF00000000ull : 0x00000000FFFFFFFFull;
#pragma unroll
    for (int i = 0; i < N - 1; i++) {
        const count_t b = __ballot((flags >> i) & 1u);
        cnt[i] = (count_t)__popcll(b);
        hcnt[i] = (count_t)__popcll(b & half_mask);
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) steps += __shfl_xor(steps, o);
    hcnt[N - 1] = steps;
    cnt[N - 1] = steps + __shfl_xor(steps, 32);
}

template <int N>
LG_DEV void wave_counts(const unsigned flags, const count_t steps, count_t (&cnt)[N]) {
    count_t hcnt[N];
    wave_counts(flags, steps, cnt, hcnt);
}

// ---------------------------------------------------------------- per workgroup: store_wave_partials, __syncthreads(), sum_wave_partials
template <typename T, int W, int N>
LG_DEV void store_wave_partials(T (&s)[W][N], const T (&v)[N]) {
    if ((threadIdx.x & 63) != 0) return;
#pragma unroll
    for (int i = 0; i < N; i++) s[threadIdx.x >> 6][i] = v[i];
}

template <typename T, int W, int N>
LG_DEV void sum_wave_partials(const T (&s)[W][N], T (&tot)[N]) {      // thread 0; wave order, which fixes the float sums
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < N; i++) { tot[i] = s[0][i]; for (int w = 1; w < W; w++) tot[i] += s[w][i]; }
}

// ---------------------------------------------------------------- a workgroup with a done env adds to the accumulators
LG_DEV void add_episode_sums(float *extras_accum, const float (&tot)[4]) {
#pragma unroll
    for (int i = 0; i < 4; i++) atomicAdd(extras_accum + i, tot[i]);
}

template <int N>
LG_DEV void add_counts(uint64_t *accum, const count_t (&tot)[N]) {     // tot[0], the done envs, is non-zero
#pragma unroll
    for (int i = 0; i < N; i++)
        if (i == 0 || tot[i] != 0) __hip_atomic_fetch_add(reinterpret_cast<count_t *>(accum) + i, tot[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------- release, ticket, acquire
LG_DEV void release_adds() {      // this thread's adds are performed before what it does next is seen; the fence's own wait is not relied upon
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

LG_DEV bool draw_last_ticket(unsigned *ticket) {      // true in the one workgroup of the launch that arrives last; it has acquired
    release_adds();
    const bool last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
    if (last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    return last;
}

// ---------------------------------------------------------------- the last workgroup publishes
// the counts of the launch, read past the L1; true when an env was done: a launch without one leaves every mean and the totals as they are
template <int N>
LG_DEV bool load_counts(uint64_t *accum, count_t (&v)[N]) {
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = __hip_atomic_load(reinterpret_cast<count_t *>(accum) + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return v[0] != 0;
}

// means[i] = v[i + 1] / v[0], totals += v (the single writer: launches on one stream), accum = 0
template <int N>
LG_DEV void publish_counts(const count_t (&v)[N], uint64_t *accum, uint64_t *totals, float *means) {
#pragma clang fp contract(off)
    const float n = (float)v[0];
#pragma unroll
    for (int i = 0; i < N - 1; i++) means[i] = (float)v[i + 1] / n;
#pragma unroll
    for (int i = 0; i < N; i++) totals[i] = totals[i] + v[i];
#pragma unroll
    for (int i = 0; i < N; i++) __hip_atomic_store(reinterpret_cast<count_t *>(accum) + i, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

LG_DEV void reset_ticket(unsigned *ticket) { __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// extras["episode"] (:298-305): episode_means[i] = sum i / count / max_episode_length_s, extras_accum = 0, when an env was done.  CHECK: the
// caller does not know that (k_dec_post has no integer counts) and the count decides; without one the accumulator is zero as it was left
template <bool CHECK>
LG_DEV void publish_episode_means(float *extras_accum, float *episode_means, const float max_episode_length_s) {
#pragma clang fp contract(off)
    const float cnt = __hip_atomic_load(extras_accum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (CHECK && !(cnt > 0.0f)) return;
    float s[3];                                                    // all loads in flight before the first store, which they cannot pass
#pragma unroll
    for (int i = 0; i < 3; i++) s[i] = __hip_atomic_load(extras_accum + 1 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int i = 0; i < 3; i++) episode_means[i] = s[i] / cnt / max_episode_length_s;
#pragma unroll
    for (int i = 0; i < 4; i++) __hip_atomic_store(extras_accum + i, 0.0f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace lg
