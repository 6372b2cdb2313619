// lg_game_act.h -- k_prey_act: both actors of a high-level game step and the command clip in one launch (include/legged_game.h: lg_game_act).
// Each role is a call of wide_actor_body (lg_policy.h); what is here is the role split and the high-level role's wave-0 epilogue.
// Included by lg_game_act.hip only, after lg_policy.h (see lg_game_common.h for the design and lg_game.h for why it is a unit of its own).
#pragma once
#include "lg_game_common.h"

namespace lg {

// Epilogue of the high-level role of k_prey_act (wave 0; lane (env, h) holds the mean m[r] and the sample v[r] of actions 4h + r): the stores
// of lg_policy_act, then exactly k_game_pre on the sample -- same expressions, contraction off -- and the optional sigma / log-prob of
// the UNCLIPPED sample (what PPO.act stores before the env clips the caller's tensor, reference :162-174).
LG_DEV void prey_command_epilogue(const PreyActArgs &G, int env, int h, bool live, const float (&m)[4], const float (&v)[4]) {
#pragma clang fp contract(off)
    const PolicyArgs &A = G.hl.base;
    const lg_game_params &P = G.P;
    float lp = 0.0f, sg[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int a = 4 * h + r;
        sg[r] = a < LG_GAME_NUM_ACTIONS ? A.std[a] : 1.0f;
        if (a < LG_GAME_NUM_ACTIONS) { const float z = (v[r] - m[r]) / sg[r]; lp += -0.5f * z * z - __logf(sg[r]) - 0.918938533f; }
    }
    lp += __shfl_xor(lp, 32);                                                                 // the env's six actions live in lanes l and l + 32
    if (!live) return;
    const size_t row = (size_t)env * LG_GAME_NUM_ACTIONS;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int a = 4 * h + r;
        if (a >= LG_GAME_NUM_ACTIONS) continue;
        A.mean[row + a] = m[r];
        if (A.actions) A.actions[row + a] = v[r];
        if (G.sigma) G.sigma[row + a] = sg[r];
    }
    float *c = G.command + row;
    if (h == 0) {
        const float c0 = game_clip(v[0], P.cmd_lin_vel_x[0], P.cmd_lin_vel_x[1]);
        const float c1 = game_clip(v[1], P.cmd_lin_vel_y[0], P.cmd_lin_vel_y[1]);
        const float c2 = P.heading_command ? game_wrap_to_pi(v[2]) : v[2];
        const float c3 = v[3];
        c[0] = c0; c[1] = c1; c[2] = c2; c[3] = c3;
        float *ll = G.ll_commands + (size_t)env * 4;
        ll[0] = c0; ll[1] = c1; ll[2] = c2; ll[3] = c3;
        if (G.log_prob) G.log_prob[env] = lp;
    } else {
        c[4] = game_clip(v[0], P.predator_lin_vel_x[0], P.predator_lin_vel_x[1]);
        c[5] = game_clip(v[1], P.predator_lin_vel_y[0], P.predator_lin_vel_y[1]);
    }
}

// wave 0's tail of the high-level role: six actions, lane (env, h) holds actions 4h .. 4h + 3 in registers 0..3
struct PreyCommandEpilogue {
    const PreyActArgs &G;
    LG_DEV void operator()(const PolicyArgs &, int env, int h, bool live, const f32x16p &y, const float (&by)[2][4], const float (&ns)[2][4]) const {
        float m[4], v[4];
#pragma unroll
        for (int r = 0; r < 4; r++) { m[r] = y[r] + by[0][r]; v[r] = m[r] + ns[0][r]; }
        prey_command_epilogue(G, env, h, live, m, v);
    }
};

__global__ void __launch_bounds__(64 * LG_PW_WAVES) k_prey_act(const PreyActArgs G) {
    __shared__ bf16x8g xa[16][2][64], xb[32][2][64];               // as k_policy_act_wide: obs / x2 in xa, x1 / x3 in xb (96 KB), the same for both roles
    const bool first = (int)blockIdx.x < G.ll_blocks;              // both roles have ll_blocks workgroups, the low-level role the first
    const int blk = first ? (int)blockIdx.x : (int)blockIdx.x - G.ll_blocks;
    if (first) wide_actor_body<15, 16, 8, 4>(G.ll, blk, xa, xb, WideNoTap{}, WideActStores{});
    else wide_actor_body<2, 16, 8, 4>(G.hl, blk, xa, xb, WideObsCopy{G.obs_copy}, PreyCommandEpilogue{G});
}

int launch_prey_act(const PreyActArgs &G, int blocks, void *stream) {
    hipLaunchKernelGGL(k_prey_act, dim3(2 * blocks), dim3(64 * LG_PW_WAVES), 0, (hipStream_t)stream, G);
    return (int)hipGetLastError();
}

}  // namespace lg
