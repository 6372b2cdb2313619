// lg_game_common.h -- what lg_game.h (k_game_pre / k_game_post and the C entry points, in lg_game_entry.hip) and lg_game_act.h (k_prey_act, in
// lg_game_act.hip) share: the clip / wrap helpers, the argument struct of k_prey_act and its launcher.  Needs lg_policy.h.
// The helpers switch floating-point contraction off inside their bodies; this header sets no file-wide pragma.
#pragma once
#include "../../include/legged_game.h"

namespace lg {

LG_DEV float game_clip(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }      // torch.clip(x, min, max)
LG_DEV float game_urange(float lo, float hi, float u) {                                       // torch_rand_float: (upper - lower) * rand + lower
#pragma clang fp contract(off)
    return (hi - lo) * u + lo;
}
LG_DEV float game_wrap_to_pi(float a) {                                                       // utils/math.py:45-48
#pragma clang fp contract(off)
    const float two_pi = 6.2831855f, pi = 3.14159274f;
    a = fmodf(a, two_pi);
    if (a != 0.0f && a < 0.0f) a += two_pi;                                                   // torch's remainder: sign of the divisor
    if (a > pi) a -= two_pi;
    return a;
}

// ------------------------------------------------------------------ both actors of a high-level step in ONE launch (lg_game_act)
// The low-level policy acts on the observation the previous low-level step left (a command reaches it one step late, reference
// high_level_game.py:177-178), so the high-level actor + clip / wrap of its output and the low-level actor are independent inside a step.
// At 2000 envs each fills 63 workgroups of a 256-CU chip: the two run side by side, workgroups split by role -- the low-level role
// (235 inputs: the longer weight stream) on the first `ll_blocks` workgroups, the high-level role (19 inputs, ~0.6 x the weights) behind it.
// The other order was timed and is no different (DESIGN.md section 5 has the figures).
// A role is a call of wide_actor_body (lg_policy.h), the function k_policy_act_wide itself calls, with the role-local workgroup index where
// the stand-alone kernel passes blockIdx.x (env base, wave share wv, k-step rotations r0..r2) and the same rand4 keying: every MFMA sees the
// operands of the stand-alone launch in the same order, the results are bit-identical (the roles are compiled with the default
// contraction, as lg_policy.h is: lg_game_act.h).
struct PreyActArgs {
    PolicyWideArgs hl, ll;                 // high-level: sampled, hl.base.actions = unclipped sample or null; low-level: deterministic
    lg_game_params P;
    float *command, *ll_commands;          // [N,6] clipped / wrapped command, [N,4] its first four columns (what k_game_pre writes)
    float *sigma, *log_prob, *obs_copy;    // optional: [N,6] broadcast std, [N] log N(sample; mean, std) summed over the actions, [N,19] the observations read
    int32_t ll_blocks;                     // workgroups per role: the low-level role takes the first `ll_blocks`, the high-level role the rest
};
int launch_prey_act(const PreyActArgs &G, int blocks, void *stream);      // lg_game_act.hip; returns the hipError_t of the launch

}  // namespace lg
