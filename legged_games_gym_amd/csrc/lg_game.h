// lg_game.h -- the predator-prey game layer around the fused low-level step (include/legged_game.h).
//
// Two element-wise kernels, one thread per env, ~250 bytes of traffic per env per step: they are bound by launch latency.  Their job is
// to keep the whole high-level step (reference legged_gym/envs/a1_game/high_level_game.py:146-241) on the device -- high-level actor,
// k_game_pre, low-level actor, k_step, k_game_post -- so it can be captured into one HIP graph.
//
// Floating point: contraction is OFF in this header, every expression rounds once per operation in the order written.  The results are then
// bit-comparable with a NumPy float32 restatement (tests/game_twin.py) except behind sqrtf / acosf, which are 1-ulp on this build.
//
// Included from lg_kernels.hip after its error helpers (fail / HIP_TRY).  The shared actor kernel behind lg_game_act, k_prey_act, lives in
// lg_game_act.h and is compiled in a translation unit of its own (lg_game_act.hip): inside lg_kernels.hip its presence alone changes hipcc's
// register allocation of the existing k_policy_act_wide instantiations (211 / 214 -> 216 / 212 VGPRs).  What both units share -- the
// clip / wrap helpers, the kernel's argument struct, its launcher -- is in lg_game_common.h.
#pragma once
#include "lg_game_common.h"

namespace lg {

#pragma clang fp contract(off)

enum { RNG_GAME_ROOT = 16, RNG_GAME_PREDATOR = 17 };      // Philox purposes; the step kernel's own root draw uses RNG_ROOT
#define LG_GAME_BLOCK 256


__global__ __launch_bounds__(LG_GAME_BLOCK) void k_game_pre(lg_game_params P, lg_game_buffers B) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * LG_GAME_BLOCK + threadIdx.x;
    if (e >= P.num_envs) return;
    float *c = B.command + (size_t)e * LG_GAME_NUM_ACTIONS;
    const float c0 = game_clip(c[0], P.cmd_lin_vel_x[0], P.cmd_lin_vel_x[1]);
    const float c1 = game_clip(c[1], P.cmd_lin_vel_y[0], P.cmd_lin_vel_y[1]);
    const float c2 = P.heading_command ? game_wrap_to_pi(c[2]) : c[2];                        // (:165) column 2, as the reference
    const float c3 = c[3];
    const float c4 = game_clip(c[4], P.predator_lin_vel_x[0], P.predator_lin_vel_x[1]);
    const float c5 = game_clip(c[5], P.predator_lin_vel_y[0], P.predator_lin_vel_y[1]);
    c[0] = c0; c[1] = c1; c[2] = c2; c[4] = c4; c[5] = c5;
    float *ll = B.ll_commands + (size_t)e * 4;                                                // (:174)
    ll[0] = c0; ll[1] = c1; ll[2] = c2; ll[3] = c3;
}

__global__ __launch_bounds__(LG_GAME_BLOCK) void k_game_post(lg_game_params P, lg_game_buffers B, int64_t step_arg) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * LG_GAME_BLOCK + threadIdx.x;
    if (e >= P.num_envs) return;
    const int64_t step = step_arg >= 0 ? step_arg : B.ll_step_counter[0];
    float *root = B.ll_root_states + (size_t)e * 13;
    float *pp = B.predator_pos + (size_t)e * 3;
    float *obs = B.obs + (size_t)e * LG_GAME_NUM_OBS;
    const float *org = B.ll_env_origins + (size_t)e * 3;

    int64_t ep_step = B.curr_episode_step[e] + 1;                                             // (:182)

    // step_predator_single_integrator (:281-283)
    float px = pp[0], py = pp[1], pz = pp[2];
    const float vx = B.command[(size_t)e * LG_GAME_NUM_ACTIONS + 4], vy = B.command[(size_t)e * LG_GAME_NUM_ACTIONS + 5];
    const float dx = P.sim_dt * vx, dy = P.sim_dt * vy;
    for (int i = 0; i < P.decimation; i++) { px = px + dx; py = py + dy; }

    float qx = root[0], qy = root[1], qz = root[2];                                           // prey_states[:, :3]
    float quat_z = root[5], quat_w = root[6];

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
        rand4(P.seed, e, step, RNG_GAME_ROOT, 0, u);
        rand4(P.seed, e, step, RNG_GAME_ROOT, 1, v);
        rand4(P.seed, e, step, RNG_GAME_PREDATOR, 0, w);
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

}  // namespace lg

extern "C" {

static int game_check(const lg_game_params *P, const lg_game_buffers *B) {
    if (!P || !B) return fail(-1, "null argument");
    if (P->num_envs < 1 || P->decimation < 0) return fail(-2, "lg_game_params: num_envs must be >= 1 and decimation >= 0");
    return 0;
}

int lg_game_pre(const lg_game_params *P, const lg_game_buffers *B, void *stream) {
    if (int rc = game_check(P, B)) return rc;
    if (!B->command || !B->ll_commands) return fail(-1, "lg_game_pre needs command and ll_commands");
    hipLaunchKernelGGL(lg::k_game_pre, dim3((P->num_envs + LG_GAME_BLOCK - 1) / LG_GAME_BLOCK), dim3(LG_GAME_BLOCK), 0, (hipStream_t)stream, *P, *B);
    HIP_TRY(hipGetLastError());
    return 0;
}

int lg_game_post(const lg_game_params *P, const lg_game_buffers *B, int64_t common_step_counter, void *stream) {
    if (int rc = game_check(P, B)) return rc;
    if (!B->command || !B->ll_root_states || !B->ll_env_origins || !B->ll_rew_buf || !B->ll_reset_buf || !B->predator_pos || !B->obs || !B->rew ||
        !B->reset_buf || !B->curr_episode_step || !B->episode_length_buf || !B->episode_sums) return fail(-1, "lg_game_post: a buffer pointer is null");
    if (common_step_counter < 0 && !B->ll_step_counter) return fail(-9, "common_step_counter = -1 needs the low-level step_counter buffer");
    hipLaunchKernelGGL(lg::k_game_post, dim3((P->num_envs + LG_GAME_BLOCK - 1) / LG_GAME_BLOCK), dim3(LG_GAME_BLOCK), 0, (hipStream_t)stream, *P, *B,
                       common_step_counter);
    HIP_TRY(hipGetLastError());
    return 0;
}

int lg_game_act(lg_policy *hl, lg_policy *ll, const lg_game_params *P, const lg_game_buffers *B, const float *hl_obs, const float *ll_obs,
                float *ll_actions, float *mean, uint64_t seed, int64_t step, const int64_t *step_counter, int32_t deterministic,
                float *sample, float *sigma, float *log_prob, float *obs_copy, void *stream) {
    if (int rc = game_check(P, B)) return rc;
    if (!hl || !ll || !hl_obs || !ll_obs || !ll_actions || !mean) return fail(-1, "null argument");
    if (!B->command || !B->ll_commands) return fail(-1, "lg_game_act needs command and ll_commands");
    const bool hl_ok = hl->wide && hl->dims[0] == LG_GAME_NUM_OBS && hl->dims[4] == LG_GAME_NUM_ACTIONS;
    const bool ll_ok = ll->wide && ll->tiles[0] == 15;
    if (g_wide_precision != 1 || !hl_ok || !ll_ok)
        return fail(-4, "the shared actor launch is compiled for the 19-512-256-128-6 / 235-512-256-128 pair at wide precision 1; use lg_policy_act x 2 + lg_game_pre");
    lg::PreyActArgs g;
    fill_policy_args(hl, g.hl.base, hl_obs, sample, mean, P->num_envs, seed, step, step_counter, deterministic);
    fill_policy_args(ll, g.ll.base, ll_obs, ll_actions, nullptr, P->num_envs, seed, step, step_counter, 1);
    for (int i = 0; i < 4; i++) {
        g.hl.wb[i] = reinterpret_cast<const lg::bf16x8g *>(hl->d_wb[i]); g.hl.bb[i] = hl->d_bb[i];
        g.ll.wb[i] = reinterpret_cast<const lg::bf16x8g *>(ll->d_wb[i]); g.ll.bb[i] = ll->d_bb[i];
    }
    g.P = *P; g.command = B->command; g.ll_commands = B->ll_commands;
    g.sigma = sigma; g.log_prob = log_prob; g.obs_copy = obs_copy;
    const int blocks = (P->num_envs + LG_PW_ENVS - 1) / LG_PW_ENVS;
    g.ll_blocks = blocks;
    HIP_TRY((hipError_t)lg::launch_prey_act(g, blocks, stream));
    return 0;
}

int lg_game_sizeof(int which) {
    switch (which) { case 0: return (int)sizeof(lg_game_params); case 1: return (int)sizeof(lg_game_buffers); default: return -1; }
}

}  // extern "C"
