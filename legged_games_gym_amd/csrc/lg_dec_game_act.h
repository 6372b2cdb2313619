// lg_dec_game_act.h -- one role of the shared actor launch of the decentralised predator-prey game: dec_actor_role<K0S, ROLE> and the wave-0
// epilogue of a sampled role, dec_command_epilogue<PREY>.  The body of k_dec_act (lg_dec_game.hip) and of k_pool_act (lg_pool_act.hip), so
// that a role computes bit-identical results in both: the second differs only in where a sampled role's weights, biases and std come from.
// Device code only; needs lg_device.h, lg_policy.h and lg_dec_game_common.h (DecActArgs).
#pragma once
#include "lg_game_common.h"    // game_clip, game_wrap_to_pi

namespace lg {

// Epilogue of a sampled role (wave 0).  All NA <= 4 actions of the agent sit in registers 0..3 of the lanes with h == 0: the stores of
// lg_policy_act, then exactly the agent's half of k_dec_pre on the sample -- same expressions, contraction off -- and the optional sigma /
// log-prob of the UNCLIPPED sample (what PPO.act stores before the env clips the caller's tensor, reference :182-189).
template <bool PREY>
LG_DEV void dec_command_epilogue(const PolicyArgs &A, const DecActAgent &O, const lg_dec_game_params &P, float *ll_commands, int env,
                                 const float (&m)[4], const float (&v)[4]) {
#pragma clang fp contract(off)
    constexpr int NA = PREY ? LG_DEC_NUM_ACTIONS_PREY : LG_DEC_NUM_ACTIONS_PRED;
    const size_t row = (size_t)env * NA;
    float lp = 0.0f;
#pragma unroll
    for (int r = 0; r < NA; r++) {
        const float sg = A.std[r];
        const float z = (v[r] - m[r]) / sg;
        lp += -0.5f * z * z - __logf(sg) - 0.918938533f;
        A.mean[row + r] = m[r];
        if (A.actions) A.actions[row + r] = v[r];
        if (O.sigma) O.sigma[row + r] = sg;
    }
    if (O.log_prob) O.log_prob[env] = lp;
    float *c = O.command + row;
    if constexpr (PREY) {
        const float c0 = game_clip(v[0], P.cmd_lin_vel_x[0], P.cmd_lin_vel_x[1]);
        const float c1 = game_clip(v[1], P.cmd_lin_vel_y[0], P.cmd_lin_vel_y[1]);
        const float c2 = P.heading_command ? game_wrap_to_pi(v[2]) : v[2];
        const float c3 = v[3];
        c[0] = c0; c[1] = c1; c[2] = c2; c[3] = c3;
        float *ll = ll_commands + (size_t)env * 4;
        ll[0] = c0; ll[1] = c1; ll[2] = c2; ll[3] = c3;
    } else {
        c[0] = game_clip(v[0], P.predator_lin_vel_x[0], P.predator_lin_vel_x[1]);
        c[1] = game_clip(v[1], P.predator_lin_vel_y[0], P.predator_lin_vel_y[1]);
    }
}

// ROLE 0: low-level actor (deterministic, stores as k_policy_act_wide), 1: prey, 2: predator.  The body of k_policy_act_wide<K0S,16,8,4>.
template <int K0S, int ROLE>
LG_DEV void dec_actor_role(const PolicyWideArgs &W, const DecActArgs &G, const int blk, bf16x8g (*xa)[2][64], bf16x8g (*xb)[2][64]) {
    const PolicyArgs &A = W.base;
    constexpr int NW = LG_PW_WAVES, H1T = 16, H2T = 8, H3T = 4;
    constexpr int T1 = H1T / NW, T2 = H2T / NW, T3 = 1;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5;
    const int wv = (wave + blk) % NW;
    const int r0 = (blk * 5) % K0S, r1 = (blk * 5) % (2 * H1T), r2 = (blk * 5) % (2 * H2T);
    const bool on2 = wv * T2 < H2T, on3 = wv * T3 < H3T;
    const int64_t step = A.step >= 0 ? A.step : (A.step_counter ? A.step_counter[0] + 1 : 0);
    int env = blk * LG_PW_ENVS + (lane & 31);
    const bool live = env < A.num_envs;
    if (!live) env = A.num_envs - 1;
    const float *o = A.obs + (size_t)env * A.num_obs;
    float *obs_copy = ROLE == 1 ? G.a_prey.obs_copy : (ROLE == 2 ? G.a_pred.obs_copy : nullptr);
    WideStream<K0S, T1> s1;
    s1.prime(W.wb[0], wv * T1, r0, lane);
    for (int s = wave; s < K0S; s += NW) {
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; i++) { const int k = 16 * s + 8 * h + i; v[i] = k < A.num_obs ? o[k] : 0.0f; }
        if (ROLE != 0 && obs_copy && live) {                       // the rollout storage's / the other ping-pong buffer's copy of what was read
#pragma unroll
            for (int i = 0; i < 8; i++) { const int k = 16 * s + 8 * h + i; if (k < A.num_obs) obs_copy[(size_t)env * A.num_obs + k] = v[i]; }
        }
        bf16x8g hi, lo;
        split8(v, hi, lo);
        xa[s][0][lane] = hi; xa[s][1][lane] = lo;
    }
    float ns[2][4], by[2][4];                                      // std * eps (0 when deterministic), output bias: the noise block of k_policy_act_wide
    if (wave == 0) {
#pragma unroll
        for (int ii = 0; ii < 2; ii++) {
            const int g = 2 * ii + h;
#pragma unroll
            for (int r = 0; r < 4; r++) { ns[ii][r] = 0.0f; by[ii][r] = 0.0f; }
            if (4 * g >= A.num_actions) continue;
            float u[4];
            rand4(A.seed ^ 0x9E3779B97F4A7C15ull, env, step, 100 + g, 0, u);
            const float rad0 = sqrtf(-2.0f * __logf(fmaxf(u[0], 1e-12f))), rad1 = sqrtf(-2.0f * __logf(fmaxf(u[2], 1e-12f)));
            float s0, c0, sn1, c1;
            __sincosf(6.2831853f * u[1], &s0, &c0);
            __sincosf(6.2831853f * u[3], &sn1, &c1);
            const float eps[4] = {rad0 * c0, rad0 * s0, rad1 * c1, rad1 * sn1};
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int a = 4 * g + r;
                if (a < A.num_actions) { by[ii][r] = W.bb[3][a]; ns[ii][r] = A.deterministic ? 0.0f : A.std[a] * eps[r]; }
            }
        }
    }
    __syncthreads();
    f32x16p a1[T1];
    s1.run(W.wb[0], xa, wv * T1, r0, lane, a1);
    WideStream<2 * H1T, T2> s2;
    if (on2) s2.prime(W.wb[1], wv * T2, r1, lane);
    __builtin_amdgcn_sched_barrier(0);
    wide_epilogue<T1>(a1, W.bb[0], xb, wv * T1, lane);
    __syncthreads();
    f32x16p a2[T2];
    WideStream<2 * H2T, T3> s3;
    if (on2) s2.run(W.wb[1], xb, wv * T2, r1, lane, a2);
    if (on3) s3.prime(W.wb[2], wv * T3, r2, lane);
    __builtin_amdgcn_sched_barrier(0);
    if (on2) wide_epilogue<T2>(a2, W.bb[1], xa, wv * T2, lane);
    __syncthreads();
    f32x16p a3[T3];
    WideStream<2 * H3T, 1> s4;
    if (on3) s3.run(W.wb[2], xa, wv * T3, r2, lane, a3);
    if (wave == 0) s4.prime(W.wb[3], 0, 0, lane);
    __builtin_amdgcn_sched_barrier(0);
    if (on3) wide_epilogue<T3>(a3, W.bb[2], xb, wv * T3, lane);
    __syncthreads();
    if (wave != 0) return;
    f32x16p y[1];
    s4.run(W.wb[3], xb, 0, 0, lane, y);
    if constexpr (ROLE != 0) {                                     // at most four actions: registers 0..3 of the lanes with h == 0
        if (h != 0 || !live) return;
        float m[4], v[4];
#pragma unroll
        for (int r = 0; r < 4; r++) { m[r] = y[0][r] + by[0][r]; v[r] = m[r] + ns[0][r]; }
        dec_command_epilogue<ROLE == 1>(A, ROLE == 1 ? G.a_prey : G.a_pred, G.P, G.ll_commands, env, m, v);
    } else {
#pragma unroll
        for (int ii = 0; ii < 2; ii++) {
            const int g = 2 * ii + h;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int a = 4 * g + r;
                if (a < A.num_actions && live) {
                    const float mm = y[0][4 * ii + r] + by[ii][r];
                    if (A.mean) A.mean[(size_t)env * A.num_actions + a] = mm;
                    A.actions[(size_t)env * A.num_actions + a] = mm + ns[ii][r];
                }
            }
        }
    }
}

}  // namespace lg
