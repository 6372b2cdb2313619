// lg_game.h -- the predator-prey game layer around the fused low-level step (include/legged_game.h).
//
// Two element-wise kernels, one thread per env, ~250 bytes of traffic per env per step: they are bound by launch latency.  Their job is
// to keep the whole high-level step (reference legged_gym/envs/a1_game/high_level_game.py:146-241) on the device -- high-level actor,
// k_game_pre, low-level actor, k_step, k_game_post -- so it can be captured into one HIP graph.
//
// Floating point: contraction is OFF in this header, every expression rounds once per operation in the order written.  The results are then
// bit-comparable with a NumPy float32 restatement (tests/game_twin.py) except behind sqrtf / acosf, which are 1-ulp on this build.
//
// The first of the entry headers of lg_game_entry.hip; includes what it uses (lg_host.h: fail / HIP_TRY, lg_policy and its fill helpers).  The
// shared actor kernel behind lg_game_act, k_prey_act, lives in lg_game_act.h and is compiled in a translation unit of its own
// (lg_game_act.hip): in one unit with the k_policy_act_wide instantiations of lg_policy_act (lg_learner.hip) its presence alone changes
// hipcc's register allocation of those (211 / 214 -> 216 / 212 VGPRs).  What both units share -- the
// clip / wrap helpers, the kernel's argument struct, its launcher -- is in lg_game_common.h.
#pragma once
#include "lg_host.h"
#include "lg_game_common.h"
#include "lg_game_post.h"      // game_post_env: the body of k_game_post, shared with the other post kernels

namespace lg {

#pragma clang fp contract(off)

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
    const int e = blockIdx.x * LG_GAME_BLOCK + threadIdx.x;
    if (e >= P.num_envs) return;
    game_post_env<false, false>(P, lg_pursuer_params{}, B, nullptr, nullptr, e, step_arg >= 0 ? step_arg : B.ll_step_counter[0], nullptr);
}

}  // namespace lg

extern "C" {

static int game_check(const lg_game_params *P, const lg_game_buffers *B) {
    if (!P || !B) return lg::fail(-1, "null argument");
    if (P->num_envs < 1 || P->decimation < 0) return lg::fail(-2, "lg_game_params: num_envs must be >= 1 and decimation >= 0");
    return 0;
}

// What every single-policy post entry point (lg_game_post, lg_pursuer_post, lg_outcome_post, lg_outcome_pursuer_post) asks of the buffers,
// after game_check; the scripted pursuer does not read `command`.
static int game_post_check(const char *who, const lg_game_buffers *B, bool need_command, int64_t common_step_counter) {
    if ((need_command && !B->command) || !B->ll_root_states || !B->ll_env_origins || !B->ll_rew_buf || !B->ll_reset_buf || !B->predator_pos || !B->obs ||
        !B->rew || !B->reset_buf || !B->curr_episode_step || !B->episode_length_buf || !B->episode_sums)
        return lg::fail(-1, "%s: a buffer pointer is null", who);
    if (common_step_counter < 0 && !B->ll_step_counter) return lg::fail(-9, "common_step_counter = -1 needs the low-level step_counter buffer");
    return 0;
}

int lg_game_pre(const lg_game_params *P, const lg_game_buffers *B, void *stream) {
    if (int rc = game_check(P, B)) return rc;
    if (!B->command || !B->ll_commands) return lg::fail(-1, "lg_game_pre needs command and ll_commands");
    hipLaunchKernelGGL(lg::k_game_pre, dim3((P->num_envs + LG_GAME_BLOCK - 1) / LG_GAME_BLOCK), dim3(LG_GAME_BLOCK), 0, (hipStream_t)stream, *P, *B);
    HIP_TRY(hipGetLastError());
    return 0;
}

int lg_game_post(const lg_game_params *P, const lg_game_buffers *B, int64_t common_step_counter, void *stream) {
    if (int rc = game_check(P, B)) return rc;
    if (int rc = game_post_check("lg_game_post", B, true, common_step_counter)) return rc;
    hipLaunchKernelGGL(lg::k_game_post, dim3((P->num_envs + LG_GAME_BLOCK - 1) / LG_GAME_BLOCK), dim3(LG_GAME_BLOCK), 0, (hipStream_t)stream, *P, *B,
                       common_step_counter);
    HIP_TRY(hipGetLastError());
    return 0;
}

int lg_game_act(lg_policy *hl, lg_policy *ll, const lg_game_params *P, const lg_game_buffers *B, const float *hl_obs, const float *ll_obs,
                float *ll_actions, float *mean, uint64_t seed, int64_t step, const int64_t *step_counter, int32_t deterministic,
                float *sample, float *sigma, float *log_prob, float *obs_copy, void *stream) {
    if (int rc = game_check(P, B)) return rc;
    if (!hl || !ll || !hl_obs || !ll_obs || !ll_actions || !mean) return lg::fail(-1, "null argument");
    if (!B->command || !B->ll_commands) return lg::fail(-1, "lg_game_act needs command and ll_commands");
    const bool hl_ok = hl->wide && hl->dims[0] == LG_GAME_NUM_OBS && hl->dims[4] == LG_GAME_NUM_ACTIONS;
    const bool ll_ok = ll->wide && ll->tiles[0] == 15;
    if (lg::wide_precision() != 1 || !hl_ok || !ll_ok)
        return lg::fail(-4, "the shared actor launch is compiled for the 19-512-256-128-6 / 235-512-256-128 pair at wide precision 1; use lg_policy_act x 2 + lg_game_pre");
    lg::PreyActArgs g;
    lg::fill_policy_args(hl, g.hl.base, hl_obs, sample, mean, P->num_envs, seed, step, step_counter, deterministic);
    lg::fill_policy_args(ll, g.ll.base, ll_obs, ll_actions, nullptr, P->num_envs, seed, step, step_counter, 1);
    lg::fill_wide_operands(hl, g.hl.wb, g.hl.bb);
    lg::fill_wide_operands(ll, g.ll.wb, g.ll.bb);
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
