// lg_dec_game.h -- C entry points of the decentralised predator-prey game (include/legged_dec_game.h).  Host code only: the kernels live in
// lg_dec_game.hip behind the launchers of lg_dec_game_common.h.  An entry header of lg_game_entry.hip; includes what it uses.
#pragma once
#include "lg_host.h"                // fail / HIP_TRY, lg_policy and its fill helpers
#include "lg_dec_game_common.h"

extern "C" {

static int dec_game_check(const lg_dec_game_params *P, const lg_dec_game_buffers *B) {
    if (!P || !B) return lg::fail(-1, "null argument");
    if (P->num_envs < 1 || P->decimation < 0) return lg::fail(-2, "lg_dec_game_params: num_envs must be >= 1 and decimation >= 0");
    return 0;
}

int lg_dec_game_pre(const lg_dec_game_params *P, const lg_dec_game_buffers *B, void *stream) {
    if (int rc = dec_game_check(P, B)) return rc;
    if (!B->command_prey || !B->command_pred || !B->ll_commands) return lg::fail(-1, "lg_dec_game_pre needs command_prey, command_pred and ll_commands");
    HIP_TRY((hipError_t)lg::launch_dec_pre(*P, *B, stream));
    return 0;
}

// what lg_dec_game_post and lg_dec_outcome_post (lg_dec_game_outcome_entry.h) require of their buffers, after dec_game_check
static int dec_game_post_check(const char *who, const lg_dec_game_params *P, const lg_dec_game_buffers *B, int64_t common_step_counter) {
    if (!B->command_pred || !B->ll_root_states || !B->ll_dof_state || !B->ll_env_origins || !B->ll_rew_buf || !B->ll_reset_buf || !B->predator_pos ||
        !B->obs_prey || !B->obs_pred || !B->rew_prey || !B->rew_pred || !B->reset_buf || !B->time_out_buf || !B->curr_episode_step ||
        !B->episode_length_buf || !B->episode_sums || !B->episode_means || !B->extras_accum || !B->extras_ticket)
        return lg::fail(-1, "%s: a buffer pointer is null", who);
    if (!(P->max_episode_length_s > 0.0f)) return lg::fail(-2, "lg_dec_game_params: max_episode_length_s must be positive");
    if (common_step_counter < 0 && !B->ll_step_counter) return lg::fail(-9, "common_step_counter = -1 needs the low-level step_counter buffer");
    return 0;
}

int lg_dec_game_post(const lg_dec_game_params *P, const lg_dec_game_buffers *B, int64_t common_step_counter, void *stream) {
    if (int rc = dec_game_check(P, B)) return rc;
    if (int rc = dec_game_post_check("lg_dec_game_post", P, B, common_step_counter)) return rc;
    HIP_TRY((hipError_t)lg::launch_dec_post(*P, *B, common_step_counter, stream));
    return 0;
}

// The arguments of k_dec_act, which k_pool_act takes too (lg_dec_game_pool_entry.h); the callers have checked the handles and the buffers.
// A null outputs struct asks for none of the optional outputs.
static void fill_dec_act_args(lg::DecActArgs &g, const lg_policy *pred, const lg_policy *prey, const lg_policy *ll, const lg_dec_game_params *P,
                              const lg_dec_game_buffers *B, const float *pred_obs, const float *prey_obs, const float *ll_obs, float *ll_actions,
                              float *mean_pred, float *mean_prey, uint64_t seed_pred, uint64_t seed_prey, int64_t step, const int64_t *step_counter,
                              int32_t deterministic_pred, int32_t deterministic_prey, const lg_dec_act_outputs *out_pred, const lg_dec_act_outputs *out_prey) {
    const lg_dec_act_outputs none = {nullptr, nullptr, nullptr, nullptr};
    const lg_dec_act_outputs &op = out_pred ? *out_pred : none, &oy = out_prey ? *out_prey : none;
    lg::fill_policy_args(ll, g.ll.base, ll_obs, ll_actions, nullptr, P->num_envs, seed_prey, step, step_counter, 1);
    lg::fill_policy_args(prey, g.prey.base, prey_obs, oy.sample, mean_prey, P->num_envs, seed_prey, step, step_counter, deterministic_prey);
    lg::fill_policy_args(pred, g.pred.base, pred_obs, op.sample, mean_pred, P->num_envs, seed_pred, step, step_counter, deterministic_pred);
    lg::fill_wide_operands(ll, g.ll.wb, g.ll.bb);
    lg::fill_wide_operands(prey, g.prey.wb, g.prey.bb);
    lg::fill_wide_operands(pred, g.pred.wb, g.pred.bb);
    g.P = *P;
    g.a_prey = {B->command_prey, oy.sigma, oy.log_prob, oy.obs_copy};
    g.a_pred = {B->command_pred, op.sigma, op.log_prob, op.obs_copy};
    g.ll_commands = B->ll_commands;
    g.blocks = (P->num_envs + LG_PW_ENVS - 1) / LG_PW_ENVS;
}

int lg_dec_game_act(lg_policy *pred, lg_policy *prey, lg_policy *ll, const lg_dec_game_params *P, const lg_dec_game_buffers *B, const float *pred_obs,
                    const float *prey_obs, const float *ll_obs, float *ll_actions, float *mean_pred, float *mean_prey, uint64_t seed_pred, uint64_t seed_prey,
                    int64_t step, const int64_t *step_counter, int32_t deterministic_pred, int32_t deterministic_prey, const lg_dec_act_outputs *out_pred,
                    const lg_dec_act_outputs *out_prey, void *stream) {
    if (int rc = dec_game_check(P, B)) return rc;
    if (!pred || !prey || !ll || !pred_obs || !prey_obs || !ll_obs || !ll_actions || !mean_pred || !mean_prey) return lg::fail(-1, "null argument");
    if (!B->command_prey || !B->command_pred || !B->ll_commands) return lg::fail(-1, "lg_dec_game_act needs command_prey, command_pred and ll_commands");
    const bool prey_ok = prey->wide && prey->dims[0] == LG_DEC_NUM_OBS_PREY && prey->dims[4] == LG_DEC_NUM_ACTIONS_PREY;
    const bool pred_ok = pred->wide && pred->dims[0] == LG_DEC_NUM_OBS_PRED && pred->dims[4] == LG_DEC_NUM_ACTIONS_PRED;
    const bool ll_ok = ll->wide && ll->tiles[0] == 15;
    if (lg::wide_precision() != 1 || !prey_ok || !pred_ok || !ll_ok)
        return lg::fail(-4, "the shared actor launch is compiled for the 3-512-256-128-2 / 16-512-256-128-4 / 235-512-256-128 triple at wide precision 1; use lg_policy_act x 3 + lg_dec_game_pre");
    if (seed_pred == seed_prey) return lg::fail(-2, "lg_dec_game_act: seed_pred and seed_prey must differ (the sampled roles share their noise purposes)");
    lg::DecActArgs g;
    fill_dec_act_args(g, pred, prey, ll, P, B, pred_obs, prey_obs, ll_obs, ll_actions, mean_pred, mean_prey, seed_pred, seed_prey, step, step_counter,
                      deterministic_pred, deterministic_prey, out_pred, out_prey);
    HIP_TRY((hipError_t)lg::launch_dec_act(g, stream));
    return 0;
}

int lg_dec_game_sizeof(int which) {
    switch (which) {
        case 0: return (int)sizeof(lg_dec_game_params);
        case 1: return (int)sizeof(lg_dec_game_buffers);
        case 2: return (int)sizeof(lg_dec_act_outputs);
        default: return -1;
    }
}

}  // extern "C"
