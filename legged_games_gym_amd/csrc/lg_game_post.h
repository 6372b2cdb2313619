// lg_game_post.h -- the per-env post stage of the predator-prey step, once, for the four kernels that run it: k_game_post (lg_game.h),
// k_pursuer_post (lg_pursuer_game.hip), k_outcome_post<> (lg_game_outcome.h) and k_dec_post (lg_dec_game.hip).  Device code only, laid out as
// the NumPy twin is (tests/game_twin.py: integrate_predator, reward, dones, reset_root, sense, observe, post): the three single-policy
// kernels are game_post_env<SCRIPTED, OUTCOME> behind an index and a bounds check; the decentralised game has its own reward, termination and
// joint reset and calls the integrator, the root reset and the observation writer.
//
// Floating point: contraction is OFF inside every body (no file-wide pragma), every expression rounds once per operation in the order
// written, so the results are bit-comparable with the twin except behind sqrtf / acosf (1 ulp on this build).  The kernels are element-wise,
// one thread per env, ~250 bytes per env: bound by launch latency, at 8 waves/SIMD while they allocate at most 64 VGPRs, so their rows in
// kernel_resources.txt may move by a few VGPRs under that ceiling without effect.  Needs lg_device.h (rand4).
#pragma once
#include "lg_game_common.h"
#include "../../include/legged_pursuer_game.h"

namespace lg {

enum { RNG_GAME_ROOT = 16, RNG_GAME_PREDATOR = 17 };      // Philox purposes; the step kernel's own root draw uses RNG_ROOT

// What a post stage holds in registers of one env: the predator's position, the prey's position and the z, w of its quaternion.
struct GamePose { float px, py, pz, qx, qy, qz, quat_z, quat_w; };

LG_DEV GamePose game_load_pose(const float *pp, const float *root) {                          // prey_states[:, :3], base_quat
    return {pp[0], pp[1], pp[2], root[0], root[1], root[2], root[5], root[6]};
}

// The correctly rounded float32 quotient n / d for integers |n| <= 2^21, 1 <= d <= 2^20, whatever the error of v_rcp_f32 (1 ulp):
// q0 = n * rcp(d) is within 2 ulp of n / d, so the residual r = n - q0 * d is a float and the fma yields it exactly; q0 + r * rcp(d)
// then differs from n / d by |r / d| * 2^-22 < 2^-21 ulp(q) before its single rounding.  n / d with d <= 2^20 is either a float
// or at least ulp / 2^21 away from every rounding boundary (a boundary is a 25-bit number m / 2^k, and |n / d - m / 2^k| >= 1 / (d 2^k)),
// so that rounding lands on the nearest float of the true quotient.  tests/test_gpu_pursuer_game.py checks every ep in 0 .. 2L.
// For any finite floats with a normal d the same step leaves |q - n / d| far below an ulp before the rounding, so n = +-d gives exactly +-1:
// game_observe needs that of the acos argument of a predator dead ahead or dead behind (the plain division, d's mantissa times its 1-ulp
// reciprocal, returns a neighbour of 1 for some d: a predator dead behind at 3 m came out 3.5e-4 rad short of pi).  0 / 0 stays NaN (0 * inf).
LG_DEV float game_quotient(float n, float d) {
    const float y = __builtin_amdgcn_rcpf(d);
    const float q0 = n * y;
    const float r = fmaf(-q0, d, n);
    return fmaf(r, y, q0);
}

// full_obs_predator('integrator') (high_level_game.py:297-315): the scripted pursuer's velocity.  The one division of the rule is made
// exact: the library is built with the 2.5-ulp fast division and every saturated velocity is a copy of the speed limit.
LG_DEV void game_pursuer_velocity(const lg_pursuer_params &Q, const int64_t ep_step, const GamePose &s, float &vx, float &vy) {
#pragma clang fp contract(off)
    const float L = (float)Q.max_episode_length;
    const float a = game_quotient(L - (float)ep_step, L);                                     // (:311)
    const float lim = Q.min_lin_vel * (1.0f - a) + Q.max_lin_vel * a;                         // (:312)
    vx = fminf(fmaxf((s.qx - s.px) * Q.gain, -lim), lim);                                     // torch.clamp: min > max returns max
    vy = fminf(fmaxf((s.qy - s.py) * Q.gain, -lim), lim);
}

// step_predator_single_integrator (:281-283)
LG_DEV void game_integrate_predator(const float sim_dt, const int decimation, const float vx, const float vy, GamePose &s) {
#pragma clang fp contract(off)
    const float dx = sim_dt * vx, dy = sim_dt * vy;
    for (int i = 0; i < decimation; i++) { s.px = s.px + dx; s.py = s.py + dy; }
}

// LowLevelGame._reset_root_states (low_level_game.py:409-432) of a done env: the root state, written to `root`, and the predator's
// placement; joints and the low-level buffers stay.  Params is lg_game_params or lg_dec_game_params (the same field names).
template <class Params>
LG_DEV void game_reset_root(const Params &P, const int e, const int64_t step, const float *org, float *root, GamePose &s) {
#pragma clang fp contract(off)
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
    s.qx = r[0]; s.qy = r[1]; s.qz = r[2]; s.quat_z = r[5]; s.quat_w = r[6];
    const float sgn = w[3] < 0.5f ? -1.0f : 1.0f;                                              // (:422-424)
    s.px = s.qx - sgn * game_urange(1.0f, 10.0f, w[0]);
    s.py = s.qy - sgn * game_urange(1.0f, 10.0f, w[1]);
    s.pz = P.predator_z;                                                                      // (:432); the z offset w[2] is drawn and overwritten
}

// What the next observation keeps of the last one: sensed positions t-2, t-1 (h), the newest one (o), the visibility flags t-2 .. t (f).
// Loaded before the reset so that the loads do not wait behind its stores; reset_idx (:345-349) clears it.
struct GameHistory {
    float h[6], o[3], f[3];
    LG_DEV void load(const float *obs) {
#pragma unroll
        for (int i = 0; i < 6; i++) h[i] = obs[3 + i];
#pragma unroll
        for (int i = 0; i < 3; i++) { o[i] = obs[9 + i]; f[i] = obs[13 + i]; }
    }
    LG_DEV void clear(const float max_rel_pos) {
#pragma unroll
        for (int i = 0; i < 6; i++) h[i] = max_rel_pos;
#pragma unroll
        for (int i = 0; i < 3; i++) { o[i] = max_rel_pos; f[i] = 0.0f; }
    }
};

// sense_predator (:427-458) + compute_observations (:388-409): obs[0..15].  What follows the 16 floats is the caller's.
LG_DEV void game_observe(const float half_fov, const GamePose &s, const GameHistory &k, float *obs) {
#pragma clang fp contract(off)
    const float rx = s.px - s.qx, ry = s.py - s.qy, rz = s.pz - s.qz;
    const float qn = fmaxf(sqrtf(s.quat_z * s.quat_z + s.quat_w * s.quat_w), 1e-9f);          // quat_apply_yaw: normalize((0, 0, z, w))
    const float yz = s.quat_z / qn, yw = s.quat_w / qn;
    const float tz = yz * 2.0f;                                                               // quat_apply(q_yaw, (1, 0, 0))
    const float fx = 1.0f - yz * tz, fy = yw * tz;
    const float dotv = fx * rx + fy * ry;
    const float denom = sqrtf(fx * fx + fy * fy) * sqrtf((rx * rx + ry * ry) + rz * rz);
    const float angle = game_wrap_to_pi(acosf(game_quotient(dotv, denom)));                   // no clamp: the reference has none
    const bool visible = fabsf(angle) <= half_fov;                                            // NaN (0/0, an argument past 1) compares false: occluded
    obs[0] = k.h[0]; obs[1] = k.h[1]; obs[2] = k.h[2]; obs[3] = k.h[3]; obs[4] = k.h[4]; obs[5] = k.h[5];
    obs[6] = k.o[0]; obs[7] = k.o[1]; obs[8] = k.o[2];
    obs[9] = visible ? rx : k.o[0]; obs[10] = visible ? ry : k.o[1]; obs[11] = visible ? rz : k.o[2];
    obs[12] = k.f[0]; obs[13] = k.f[1]; obs[14] = k.f[2]; obs[15] = visible ? 1.0f : 0.0f;
}

// One env of the single-policy post stage (HighLevelGame.step after ll_env.step, :182-241).  SCRIPTED: the predator's velocity comes from
// the scripted rule (and goes to the optional `predator_command` [N,2]) instead of columns 4:6 of `command`; Q is read only then.
// OUTCOME: returns the flags of a done env as bits 0..5 (done, captured, prey_out, predator_out, fell, survived), 0 for an env that goes
// on, and `*steps` receives the episode's length in high-level steps (done envs only); without it the result is 0 and `ll_time_out_buf`
// and `steps` are not touched.
template <bool SCRIPTED, bool OUTCOME>
LG_DEV unsigned game_post_env(const lg_game_params &P, const lg_pursuer_params &Q, const lg_game_buffers &B, float *predator_command,
                              const uint8_t *ll_time_out_buf, const int e, const int64_t step, unsigned long long *steps) {
#pragma clang fp contract(off)
    float *root = B.ll_root_states + (size_t)e * 13;
    float *pp = B.predator_pos + (size_t)e * 3;
    float *obs = B.obs + (size_t)e * LG_GAME_NUM_OBS;
    const float *org = B.ll_env_origins + (size_t)e * 3;

    int64_t ep_step = B.curr_episode_step[e] + 1;                                             // (:182)
    GamePose s = game_load_pose(pp, root);

    float vx, vy;
    if constexpr (SCRIPTED) {
        game_pursuer_velocity(Q, ep_step, s, vx, vy);
        if (predator_command) { predator_command[(size_t)e * 2] = vx; predator_command[(size_t)e * 2 + 1] = vy; }
    } else {
        vx = B.command[(size_t)e * LG_GAME_NUM_ACTIONS + 4]; vy = B.command[(size_t)e * LG_GAME_NUM_ACTIONS + 5];
    }
    game_integrate_predator(P.sim_dt, P.decimation, vx, vy, s);

    // compute_reward (:364-372)
    {
        const float rx = s.px - s.qx, ry = s.py - s.qy, rz = s.pz - s.qz;
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
    const bool ll_reset = B.ll_reset_buf[e] != 0;
    bool ll_time_out = false;
    if constexpr (OUTCOME) ll_time_out = ll_time_out_buf[e] != 0;
    {
        const float ax = s.qx - s.px, ay = s.qy - s.py;
        captured = sqrtf(ax * ax + ay * ay) < P.capture_dist;
        if (P.env_radius >= 0.0f) {
            const float bx = s.qx - org[0], by = s.qy - org[1], cx = s.px - org[0], cy = s.py - org[1];
            prey_out = sqrtf(bx * bx + by * by) > P.env_radius;
            predator_out = sqrtf(cx * cx + cy * cy) > P.env_radius;
        }
    }
    const bool done = captured || prey_out || predator_out || ll_reset;
    unsigned flags = 0;

    GameHistory k;
    k.load(obs);
    if (done) {
        if constexpr (OUTCOME) {
            flags = 1u | (captured ? 2u : 0u) | (prey_out ? 4u : 0u) | (predator_out ? 8u : 0u) | ((ll_reset && !ll_time_out) ? 16u : 0u) |
                    ((ll_reset && ll_time_out) ? 32u : 0u);
            *steps = (unsigned long long)ep_step;
        }
        game_reset_root(P, e, step, org, root, s);
        k.clear(P.max_rel_pos);                                                               // HighLevelGame.reset_idx (:345-349)
        ep_step = 0;
        B.episode_length_buf[e] = 0;
    }
    B.curr_episode_step[e] = ep_step;
    B.reset_buf[e] = done ? 1 : 0;
    pp[0] = s.px; pp[1] = s.py; pp[2] = s.pz;

    game_observe(P.half_fov, s, k, obs);
    obs[16] = s.qx - s.px; obs[17] = s.qy - s.py; obs[18] = s.qz - s.pz;
    return flags;
}

}  // namespace lg
