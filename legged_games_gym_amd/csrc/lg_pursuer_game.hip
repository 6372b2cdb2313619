// lg_pursuer_game.hip -- k_pursuer_post: the post stage of the predator-prey game with the reference's scripted pursuer
// (include/legged_pursuer_game.h; reference high_level_game.py:265-324 with `command=None`).  A translation unit of its own, reached through
// launch_pursuer_post, so that the code hipcc generates for the kernels of lg_kernels.hip does not depend on it (see lg_game.h).  The C
// entry points are in lg_pursuer_game.h (lg_kernels.hip).
//
// The body restates k_game_post (lg_game.h) with the predator's velocity computed in place of the two loads from `command`; sharing the
// body would move k_game_post's register allocation, whose row in kernel_resources.txt is pinned.  Floating point: contraction is OFF,
// every expression rounds once per operation in the order written, so the results are bit-comparable with the NumPy float32 restatement
// (tests/pursuer_twin.py) except behind sqrtf / acosf (1 ulp on this build).  The one division of the rule, (L - ep) / L, is made exact
// (pursuer_quotient): the library is built with the 2.5-ulp fast division and every saturated velocity is a copy of the speed limit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define LG_POLICY_BLOCKS_ONLY      // lg_policy.h (which lg_game_common.h needs) without its two non-template pack kernels
#include "lg_device.h"
#include "lg_policy.h"
#include "lg_game_common.h"
#include "../../include/legged_pursuer_game.h"

namespace lg {

enum { RNG_PURSUER_ROOT = 16, RNG_PURSUER_PREDATOR = 17 };      // Philox purposes: as k_game_post (lg_game.h)
#define LG_PURSUER_BLOCK 256

// The correctly rounded float32 quotient n / d for integers |n| <= 2^21, 1 <= d <= 2^20, whatever the error of v_rcp_f32 (1 ulp):
// q0 = n * rcp(d) is within 2 ulp of n / d, so the residual r = n - q0 * d is a float and the fma yields it exactly; q0 + r * rcp(d)
// then differs from n / d by |r / d| * 2^-22 < 2^-21 ulp(q) before its single rounding.  n / d with d <= 2^20 is either a float
// or at least ulp / 2^21 away from every rounding boundary (a boundary is a 25-bit number m / 2^k, and |n / d - m / 2^k| >= 1 / (d 2^k)),
// so that rounding lands on the nearest float of the true quotient.  tests/test_gpu_pursuer_game.py checks every ep in 0 .. 2L.
LG_DEV float pursuer_quotient(float n, float d) {
    const float y = __builtin_amdgcn_rcpf(d);
    const float q0 = n * y;
    const float r = fmaf(-q0, d, n);
    return fmaf(r, y, q0);
}

__global__ __launch_bounds__(LG_PURSUER_BLOCK) void k_pursuer_post(lg_game_params P, lg_pursuer_params Q, lg_game_buffers B, float *predator_command,
                                                                  int64_t step_arg) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * LG_PURSUER_BLOCK + threadIdx.x;
    if (e >= P.num_envs) return;
    const int64_t step = step_arg >= 0 ? step_arg : B.ll_step_counter[0];
    float *root = B.ll_root_states + (size_t)e * 13;
    float *pp = B.predator_pos + (size_t)e * 3;
    float *obs = B.obs + (size_t)e * LG_GAME_NUM_OBS;
    const float *org = B.ll_env_origins + (size_t)e * 3;

    int64_t ep_step = B.curr_episode_step[e] + 1;                                             // (:182)

    float px = pp[0], py = pp[1], pz = pp[2];
    float qx = root[0], qy = root[1], qz = root[2];                                           // prey_states[:, :3]
    float quat_z = root[5], quat_w = root[6];

    // full_obs_predator('integrator') (:297-315)
    const float L = (float)Q.max_episode_length;
    const float a = pursuer_quotient(L - (float)ep_step, L);                                  // (:311)
    const float lim = Q.min_lin_vel * (1.0f - a) + Q.max_lin_vel * a;                         // (:312)
    const float vx = fminf(fmaxf((qx - px) * Q.gain, -lim), lim);                             // torch.clamp: min > max returns max
    const float vy = fminf(fmaxf((qy - py) * Q.gain, -lim), lim);
    if (predator_command) { predator_command[(size_t)e * 2] = vx; predator_command[(size_t)e * 2 + 1] = vy; }

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

    // dones (:197-236)
    bool done;
    {
        const float ax = qx - px, ay = qy - py;
        done = sqrtf(ax * ax + ay * ay) < P.capture_dist;
        if (P.env_radius >= 0.0f) {
            const float bx = qx - org[0], by = qy - org[1], cx = px - org[0], cy = py - org[1];
            done = done || sqrtf(bx * bx + by * by) > P.env_radius || sqrtf(cx * cx + cy * cy) > P.env_radius;
        }
        done = done || B.ll_reset_buf[e] != 0;
    }

    float o9 = obs[9], o10 = obs[10], o11 = obs[11];                                           // newest sensed position
    float h[6] = {obs[3], obs[4], obs[5], obs[6], obs[7], obs[8]};
    float f13 = obs[13], f14 = obs[14], f15 = obs[15];
    if (done) {
        // LowLevelGame._reset_root_states (low_level_game.py:409-432): the root state only; joints and the low-level buffers stay
        float u[4], v[4], w[4];
        rand4(P.seed, e, step, RNG_PURSUER_ROOT, 0, u);
        rand4(P.seed, e, step, RNG_PURSUER_ROOT, 1, v);
        rand4(P.seed, e, step, RNG_PURSUER_PREDATOR, 0, w);
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
}

int launch_pursuer_post(const lg_game_params &P, const lg_pursuer_params &Q, const lg_game_buffers &B, float *predator_command, int64_t step,
                        void *stream) {
    hipLaunchKernelGGL(k_pursuer_post, dim3((P.num_envs + LG_PURSUER_BLOCK - 1) / LG_PURSUER_BLOCK), dim3(LG_PURSUER_BLOCK), 0, (hipStream_t)stream,
                       P, Q, B, predator_command, step);
    return (int)hipGetLastError();
}

}  // namespace lg
