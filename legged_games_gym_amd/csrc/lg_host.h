// lg_host.h -- what the three translation units with C entry points share on the host: lg_kernels.hip (the simulator, on an lg_sim handle),
// lg_learner.hip (fused actor and PPO learner) and lg_game_entry.hip (the game layers).  Declarations and HIP_TRY only; each name's home is
// noted beside it.
#pragma once
#include "lg_policy.h"         // PolicyArgs, bf16x8g

namespace lg {

// Sets the thread's error text, the one lg_last_error() returns whichever unit failed, and returns `code` (lg_kernels.hip).
int fail(int code, const char *fmt, const char *arg = "");
// lg_mlp_wide_set_precision's switch: 0 = f32 MFMA kernels, 1 = split-bf16 kernels, learner GEMMs and wide actors alike (lg_learner.hip)
int wide_precision();
// lg_policy_act for the flat 48-128-64-32 actor, k_policy_act<3,8,4,2>; returns the hipError_t of the launch (lg_kernels.hip)
int launch_policy_act_flat(const PolicyArgs &A, void *stream);

}  // namespace lg

#define HIP_TRY(x) do { hipError_t _e = (x); if (_e != hipSuccess) return lg::fail(-10, "HIP error: %s", hipGetErrorString(_e)); } while (0)

struct lg_policy {             // created and destroyed by lg_policy_create / lg_policy_destroy (lg_learner.hip)
    int32_t dims[5];
    int     tiles[4];          // input tiles of layer 0, then hidden widths / 16
    float  *d_w[4], *d_b[4], *d_std;
    int     device;
    // wide actors (hidden 512-256-128): split-bf16 operand stream of k_policy_act_wide next to the f32 one
    bool    wide;
    int     wide_ks[4], wide_ot[4];     // k-steps of 16 / output tiles of 32 per layer
    __bf16 *d_wb[4];
    float  *d_bb[4];
};

namespace lg {

// the arguments of k_policy_act / the `base` of a wide actor's, from a handle (lg_learner.hip)
void fill_policy_args(const lg_policy *p, PolicyArgs &a, const float *obs, float *actions, float *mean, int32_t num_envs, uint64_t seed,
                      int64_t step, const int64_t *step_counter, int32_t deterministic);
// the split-bf16 operand stream of a wide handle: the wb / bb of a PolicyWideArgs or of a pool's table row (lg_learner.hip)
void fill_wide_operands(const lg_policy *p, const bf16x8g *(&wb)[4], const float *(&bb)[4]);

}  // namespace lg
