// lg_dec_game_act.h -- one role of the shared actor launch of the decentralised predator-prey game: dec_actor_role<ROLE>, a call of
// wide_actor_body (lg_policy.h) with the role's observation tap and wave-0 epilogue, dec_command_epilogue<PREY>.  The body of k_dec_act
// (lg_dec_game.hip) and of k_pool_act (lg_pool_act.hip): the second differs only in where a sampled role's weights, biases and std come from.
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

// wave 0's tail of a sampled role: at most four actions, registers 0..3 of the lanes with h == 0
template <bool PREY> struct DecCommandEpilogue {
    const DecActArgs &G;
    LG_DEV void operator()(const PolicyArgs &A, int env, int h, bool live, const f32x16p &y, const float (&by)[2][4], const float (&ns)[2][4]) const {
        if (h != 0 || !live) return;
        float m[4], v[4];
#pragma unroll
        for (int r = 0; r < 4; r++) { m[r] = y[r] + by[0][r]; v[r] = m[r] + ns[0][r]; }
        dec_command_epilogue<PREY>(A, PREY ? G.a_prey : G.a_pred, G.P, G.ll_commands, env, m, v);
    }
};

// ROLE 0: low-level actor (deterministic, the stores of lg_policy_act), 1: prey, 2: predator.  W holds the role's operands: those of G, or
// a pool member's (lg_pool_act.hip).
template <int ROLE>
LG_DEV void dec_actor_role(const PolicyWideArgs &W, const DecActArgs &G, const int blk, bf16x8g (*xa)[2][64], bf16x8g (*xb)[2][64]) {
    if constexpr (ROLE == 0) wide_actor_body<15, 16, 8, 4>(W, blk, xa, xb, WideNoTap{}, WideActStores{});
    else wide_actor_body<1, 16, 8, 4>(W, blk, xa, xb, WideObsCopy{ROLE == 1 ? G.a_prey.obs_copy : G.a_pred.obs_copy}, DecCommandEpilogue<ROLE == 1>{G});
}

}  // namespace lg
