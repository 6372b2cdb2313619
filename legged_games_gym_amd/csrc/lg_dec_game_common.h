// lg_dec_game_common.h -- what lg_game_entry.hip (the C entry points of include/legged_dec_game.h in lg_dec_game.h), lg_learner.hip (the
// lg_policy_act dispatch) and lg_dec_game.hip (the kernels) share: the launchers.  Needs lg_policy.h.  The kernels are a translation unit of their own for the reason
// lg_game_act.hip is one: a kernel built from the wide actor blocks next to the lg_policy_act dispatch moves hipcc's register allocation of the
// k_policy_act_wide instantiations there (lg_game.h).
#pragma once
#include "../../include/legged_dec_game.h"

namespace lg {

// each returns the hipError_t of its launch
int launch_dec_pre(const lg_dec_game_params &P, const lg_dec_game_buffers &B, void *stream);
int launch_dec_post(const lg_dec_game_params &P, const lg_dec_game_buffers &B, int64_t step, void *stream);
// lg_policy_act for actors with ONE input tile (1..16 observations, hidden 512-256-128): k_policy_act<1,32,16,8> / k_policy_act_wide<1,16,8,4>
int launch_policy_act_one_tile(const PolicyArgs &A, void *stream);
int launch_policy_act_wide_one_tile(const PolicyWideArgs &W, void *stream);


// ------------------------------------------------------------------ the three actors of a decentralised game step in ONE launch (lg_dec_game_act)
// As k_prey_act (lg_game_common.h): the low-level policy reads the observation the previous low-level step left, and the two agents read
// their own observation buffers, so nothing in one actor depends on another inside a step.  Workgroups are split by role: the low-level
// role (235 inputs, deterministic) on the first `blocks` workgroups, then the prey role (16 inputs, sampled), then the predator role
// (3 inputs, sampled).  A role is a call of wide_actor_body (lg_policy.h), as k_policy_act_wide is, with the role-local workgroup index and
// its own seed: every MFMA sees the operands of the stand-alone launch in the same order.  Each sampled role's wave-0 epilogue does its
// agent's half of k_dec_pre in registers.
struct DecActAgent {
    float *command;                        // [N, actions] clipped (/ wrapped) command: what k_dec_pre leaves in the caller's tensor
    float *sigma, *log_prob, *obs_copy;    // optional: [N, actions] broadcast std, [N] log N(sample; mean, std) summed over the actions, [N, obs] the observations read
};
struct DecActArgs {
    PolicyWideArgs ll, prey, pred;         // ll deterministic; prey / pred sampled, base.actions = unclipped sample or null, base.mean required
    lg_dec_game_params P;
    DecActAgent a_prey, a_pred;
    float *ll_commands;                    // [N,4] the prey's clipped command (what k_dec_pre writes)
    int32_t blocks;                        // workgroups per role
};
int launch_dec_act(const DecActArgs &G, void *stream);

}  // namespace lg
