// lg_game_outcome.h -- k_outcome_post<SCRIPTED>: the post stage of the predator-prey game with the outcome statistics of
// include/legged_game_outcome.h.  SCRIPTED = false restates k_game_post (lg_game.h), SCRIPTED = true k_pursuer_post (lg_pursuer_game.hip):
// the same expressions in the same order with the same Philox keying, so everything those kernels write comes out bit-identical.  The body
// is restated, not shared: a neighbour in their translation units moves hipcc's register allocation of kernels whose rows in
// kernel_resources.txt are pinned.  Included from lg_game_outcome.hip only.
//
// The addition: where the plain kernels fold the causes of an episode's end into `done`, this one keeps them apart, counts them over the
// launch with integers only -- ballot + popcount per wave, LDS per workgroup, one 64-bit agent-scope atomic add per value and workgroup --
// and lets the workgroup that draws the last ticket publish means and totals (the scheme of k_dec_post, lg_dec_game.hip).
#pragma once
#include "lg_game_common.h"
#include "../../include/legged_game_outcome.h"

namespace lg {

enum { RNG_OUTCOME_ROOT = 16, RNG_OUTCOME_PREDATOR = 17 };      // Philox purposes: as k_game_post (lg_game.h)
#define LG_OUTCOME_BLOCK 256
#define LG_OUTCOME_WAVES (LG_OUTCOME_BLOCK / 64)

// The correctly rounded float32 quotient n / d of k_pursuer_post (lg_pursuer_game.hip: pursuer_quotient, with the proof).
LG_DEV float outcome_quotient(float n, float d) {
    const float y = __builtin_amdgcn_rcpf(d);
    const float q0 = n * y;
    const float r = fmaf(-q0, d, n);
    return fmaf(r, y, q0);
}

// One env of the post stage.  Returns the flags of a done env as bits 0..5 (done, captured, prey_out, predator_out, fell, survived), 0 for an
// env that goes on; `steps` receives the episode's length in high-level steps (done envs only).
template <bool SCRIPTED>
LG_DEV unsigned outcome_post_env(const lg_game_params &P, const lg_pursuer_params &Q, const lg_game_buffers &B, const uint8_t *ll_time_out_buf,
                                 float *predator_command, const int e, const int64_t step, unsigned long long &steps) {
#pragma clang fp contract(off)
    float *root = B.ll_root_states + (size_t)e * 13;
    float *pp = B.predator_pos + (size_t)e * 3;
    float *obs = B.obs + (size_t)e * LG_GAME_NUM_OBS;
    const float *org = B.ll_env_origins + (size_t)e * 3;

    int64_t ep_step = B.curr_episode_step[e] + 1;                                             // (:182)

    float px = pp[0], py = pp[1], pz = pp[2];
    float qx = root[0], qy = root[1], qz = root[2];                                           // prey_states[:, :3]
    float quat_z = root[5], quat_w = root[6];

    float vx, vy;
    if constexpr (SCRIPTED) {
        // full_obs_predator('integrator') (:297-315)
        const float L = (float)Q.max_episode_length;
        const float a = outcome_quotient(L - (float)ep_step, L);                              // (:311)
        const float lim = Q.min_lin_vel * (1.0f - a) + Q.max_lin_vel * a;                     // (:312)
        vx = fminf(fmaxf((qx - px) * Q.gain, -lim), lim);                                     // torch.clamp: min > max returns max
        vy = fminf(fmaxf((qy - py) * Q.gain, -lim), lim);
        if (predator_command) { predator_command[(size_t)e * 2] = vx; predator_command[(size_t)e * 2 + 1] = vy; }
    } else {
        vx = B.command[(size_t)e * LG_GAME_NUM_ACTIONS + 4]; vy = B.command[(size_t)e * LG_GAME_NUM_ACTIONS + 5];
    }

    // step_predator_single_integrator (:281-283)
    const float dx = P.sim_dt * vx, dy = P.sim_dt * vy;
    for (int i = 0; i < P.decimation; i++) { px = px + dx; py = py + dy; }

    // compute_reward (:364-372)
    {
        const float rx = px - qx, ry = py - qy, rz = pz - qz;
        const float d = sqrtf((rx * rx + ry * ry) + rz * rz);
        float rew = P.ll_rew_weight * B.ll_rew_buf[e];
        const float ev = d * P.scale_evasion_dt, pu = (-d) * P.scale_pursuit_dt;
        rew = rew + ev;
        rew = rew + pu;
        B.episode_sums[e] = B.episode_sums[e] + ev;
        B.episode_sums[(size_t)P.num_envs + e] = B.episode_sums[(size_t)P.num_envs + e] + pu;
        if (P.only_positive_rewards) rew = fmaxf(rew, 0.0f);
        B.rew[e] = rew;
    }

    // dones (:197-236), the causes kept apart
    bool captured, prey_out = false, predator_out = false;
    const bool ll_reset = B.ll_reset_buf[e] != 0, ll_time_out = ll_time_out_buf[e] != 0;
    {
        const float ax = qx - px, ay = qy - py;
        captured = sqrtf(ax * ax + ay * ay) < P.capture_dist;
        if (P.env_radius >= 0.0f) {
            const float bx = qx - org[0], by = qy - org[1], cx = px - org[0], cy = py - org[1];
            prey_out = sqrtf(bx * bx + by * by) > P.env_radius;
            predator_out = sqrtf(cx * cx + cy * cy) > P.env_radius;
        }
    }
    const bool done = captured || prey_out || predator_out || ll_reset;
    unsigned flags = 0;

    float o9 = obs[9], o10 = obs[10], o11 = obs[11];                                           // newest sensed position
    float h[6] = {obs[3], obs[4], obs[5], obs[6], obs[7], obs[8]};
    float f13 = obs[13], f14 = obs[14], f15 = obs[15];
    if (done) {
        flags = 1u | (captured ? 2u : 0u) | (prey_out ? 4u : 0u) | (predator_out ? 8u : 0u) | ((ll_reset && !ll_time_out) ? 16u : 0u) |
                ((ll_reset && ll_time_out) ? 32u : 0u);
        steps = (unsigned long long)ep_step;
        // LowLevelGame._reset_root_states (low_level_game.py:409-432): the root state only; joints and the low-level buffers stay
        float u[4], v[4], w[4];
        rand4(P.seed, e, step, RNG_OUTCOME_ROOT, 0, u);
        rand4(P.seed, e, step, RNG_OUTCOME_ROOT, 1, v);
        rand4(P.seed, e, step, RNG_OUTCOME_PREDATOR, 0, w);
        float r[13];
#pragma unroll
        for (int i = 0; i < 13; i++) r[i] = P.base_init_state[i];
        r[0] = r[0] + org[0]; r[1] = r[1] + org[1]; r[2] = r[2] + org[2];
        if (P.custom_origins) { r[0] = r[0] + game_urange(-1.0f, 1.0f, u[0]); r[1] = r[1] + game_urange(-1.0f, 1.0f, u[1]); }
        r[7] = game_urange(-0.5f, 0.5f, u[2]); r[8] = game_urange(-0.5f, 0.5f, u[3]);
        r[9] = game_urange(-0.5f, 0.5f, v[0]); r[10] = game_urange(-0.5f, 0.5f, v[1]);
        r[11] = game_urange(-0.5f, 0.5f, v[2]); r[12] = game_urange(-0.5f, 0.5f, v[3]);
#pragma unroll
        for (int i = 0; i < 13; i++) root[i] = r[i];
        qx = r[0]; qy = r[1]; qz = r[2]; quat_z = r[5]; quat_w = r[6];
        const float sgn = w[3] < 0.5f ? -1.0f : 1.0f;                                          // (:422-424)
        px = qx - sgn * game_urange(1.0f, 10.0f, w[0]);
        py = qy - sgn * game_urange(1.0f, 10.0f, w[1]);
        pz = P.predator_z;                                                                    // (:432); the z offset w[2] is drawn and overwritten
        // HighLevelGame.reset_idx (:345-349)
        o9 = o10 = o11 = P.max_rel_pos;
#pragma unroll
        for (int i = 0; i < 6; i++) h[i] = P.max_rel_pos;
        f13 = f14 = f15 = 0.0f;
        ep_step = 0;
        B.episode_length_buf[e] = 0;
    }
    B.curr_episode_step[e] = ep_step;
    B.reset_buf[e] = done ? 1 : 0;
    pp[0] = px; pp[1] = py; pp[2] = pz;

    // sense_predator (:427-458) + compute_observations (:388-409)
    const float rx = px - qx, ry = py - qy, rz = pz - qz;
    const float qn = fmaxf(sqrtf(quat_z * quat_z + quat_w * quat_w), 1e-9f);                  // quat_apply_yaw: normalize((0, 0, z, w))
    const float yz = quat_z / qn, yw = quat_w / qn;
    const float tz = yz * 2.0f;                                                               // quat_apply(q_yaw, (1, 0, 0))
    const float fx = 1.0f - yz * tz, fy = yw * tz;
    const float dotv = fx * rx + fy * ry;
    const float denom = sqrtf(fx * fx + fy * fy) * sqrtf((rx * rx + ry * ry) + rz * rz);
    const float angle = game_wrap_to_pi(acosf(dotv / denom));
    const bool visible = fabsf(angle) <= P.half_fov;                                          // NaN (0/0) compares false: occluded
    obs[0] = h[0]; obs[1] = h[1]; obs[2] = h[2]; obs[3] = h[3]; obs[4] = h[4]; obs[5] = h[5];
    obs[6] = o9; obs[7] = o10; obs[8] = o11;
    obs[9] = visible ? rx : o9; obs[10] = visible ? ry : o10; obs[11] = visible ? rz : o11;
    obs[12] = f13; obs[13] = f14; obs[14] = f15; obs[15] = visible ? 1.0f : 0.0f;
    obs[16] = qx - px; obs[17] = qy - py; obs[18] = qz - pz;
    return flags;
}

template <bool SCRIPTED>
__global__ __launch_bounds__(LG_OUTCOME_BLOCK) void k_outcome_post(lg_game_params P, lg_pursuer_params Q, lg_game_buffers B, lg_outcome_buffers O,
                                                                  float *predator_command, int64_t step_arg) {
#pragma clang fp contract(off)
    __shared__ unsigned long long s_part[LG_OUTCOME_WAVES][LG_OUTCOME_NUM_COUNTS];
    const int e = blockIdx.x * LG_OUTCOME_BLOCK + threadIdx.x;
    unsigned flags = 0;
    unsigned long long steps = 0;
    if (e < P.num_envs)
        flags = outcome_post_env<SCRIPTED>(P, Q, B, O.ll_time_out_buf, predator_command, e, step_arg >= 0 ? step_arg : B.ll_step_counter[0], steps);

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
