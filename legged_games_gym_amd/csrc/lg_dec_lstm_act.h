// lg_dec_lstm_act.h -- what the two recurrent policy stages of dec_high_level_game share: the kernel arguments of the cell launch and of the
// actor launch, the sampled role of the actor launch, and the host code that sizes and fills them.  lg_dec_game_lstm_act.hip
// (liblegged_dec_game_recurrent.so: k_dec_lstm_cell, k_dec_game_lstm_act) and lg_dec_pool_lstm_act.hip (liblegged_dec_pool_recurrent.so:
// k_dec_pool_lstm_cell, k_dec_pool_lstm_act) are each ONE translation unit that includes it; nothing here is exported.
// Needs lg_device.h, lg_policy.h, lg_host.h (struct lg_policy), lg_dec_game_common.h (DecActAgent), lg_dec_game_act.h
// (dec_command_epilogue), lg_recurrent.h, lg_lstm_actor_body.h and <hip/hip_runtime.h>.  The units' host code also reads lg_lib_error.h
// (raise_lds_limit) and lg_memory_host.h (cell_lds_bytes, fill_lstm_role, fill_lstm_actor_args).
#pragma once
#include "../../include/legged_recurrent.h"      // LG_LSTM_MAX_IN, LG_LSTM_MAX_HIDDEN

namespace lg {

// ------------------------------------------------------------------ the cell launch
struct DecLstmArgs {
    LstmRole role[4];              // predator actor / critic memory, prey actor / critic memory; only the present ones are filled
    const uint8_t *reset;
    int32_t num_envs, blocks;      // workgroups per present role
    uint32_t order, _pad;          // two bits per slot: the role of workgroups slot * blocks .. (slot + 1) * blocks - 1
};

static const int LSTM_MAX_KSTEPS = (LG_LSTM_MAX_IN + LG_LSTM_MAX_HIDDEN) / 2;

// ------------------------------------------------------------------ the actor launch
struct DecGameLstmActArgs {
    PolicyWideArgs ll;                     // low-level role: deterministic
    LstmActorArgs prey, pred;              // sampled roles: .actions = the unclipped sample or null, .mean required
    lg_dec_game_params P;
    DecActAgent a_prey, a_pred;            // command, sigma, log_prob, obs_copy
    const float *prey_obs, *pred_obs;      // [N,16] / [N,3], read only for obs_copy
    float *ll_commands;                    // [N,4] the prey's clipped command (what k_dec_pre writes)
    int32_t blocks, _pad;                  // workgroups per role: low-level, prey, predator
};

// last layer of a sampled role: the mean of action `unit` of row `row` into ms[32][16]
struct DecMeansToLds {
    float *ms;
    LG_DEV void operator()(const LstmActorArgs &, int, int row, int unit, float m, const float *) const { ms[row * 16 + unit] = m; }
};

// One sampled role's workgroup: env rows 32 blk .. 32 blk + 31.  smem: float xa[max_width][LG_LSTM_LD], xb[the same], ns[32][16], ms[32][16].
template <bool PREY>
LG_DEV void dec_lstm_actor_role(const LstmActorArgs &A, const DecActAgent &O, const float *obs, const lg_dec_game_params &P, float *ll_commands,
                                const int blk, char *smem) {
    constexpr int NOBS = PREY ? LG_DEC_NUM_OBS_PREY : LG_DEC_NUM_OBS_PRED;
    float *xa = reinterpret_cast<float *>(smem), *xb = xa + (size_t)A.max_width * LG_LSTM_LD, *ns = xb + (size_t)A.max_width * LG_LSTM_LD, *ms = ns + 32 * 16;
    const int tid = (int)threadIdx.x, env0 = 32 * blk;
    if (O.obs_copy) {                                              // the observations the memories read, for the storage
        for (int e = tid; e < 32 * NOBS; e += 64 * LG_PW_WAVES) {
            const size_t at = (size_t)env0 * NOBS + e;
            if (at < (size_t)A.num_envs * NOBS) O.obs_copy[at] = obs[at];
        }
    }
    lstm_actor_body<LG_PW_WAVES, 16>(A, blk, xa, xb, ns, DecMeansToLds{ms});   // (ends in a barrier: ms and ns are complete)
    if (tid < 32 && env0 + tid < A.num_envs) {
        // what DecCommandEpilogue hands dec_command_epilogue: the agent's means and mean + noise (registers past the agent's actions are not read)
        PolicyArgs S = {};
        S.std = A.std; S.actions = A.actions; S.mean = A.mean;
        float m[4], v[4];
#pragma unroll
        for (int r = 0; r < 4; r++) { m[r] = ms[tid * 16 + r]; v[r] = m[r] + ns[tid * 16 + r]; }
        dec_command_epilogue<PREY>(S, O, P, ll_commands, env0 + tid, m, v);
    }
}

// ONE dynamic block of the actor launch, carved per role:
//   low-level role    bf16x8g xa[16][2][64], xb[32][2][64]                               96 KB, as k_policy_act_wide
//   sampled roles     float xa[max_width][LG_LSTM_LD], xb[the same], ns[32][16], ms[32][16]
static size_t dec_game_lstm_lds_bytes(const int max_width) {
    const size_t hl = ((size_t)2 * max_width * LG_LSTM_LD + 32 * 16 + 32 * 16) * sizeof(float), ll = 98304;
    return hl > ll ? hl : ll;
}

// the low-level role: what fill_policy_args / fill_wide_operands do for lg_policy_act(ll, deterministic = 1)
static void fill_ll_role_args(PolicyWideArgs &W, const lg_policy *ll, const float *ll_obs, float *ll_actions, const int num_envs, const uint64_t seed,
                              const int64_t step, const int64_t *step_counter) {
    PolicyArgs &a = W.base;
    a.obs = ll_obs; a.actions = ll_actions; a.mean = nullptr; a.std = ll->d_std; a.step_counter = step_counter; a.step = step; a.seed = seed;
    a.num_envs = num_envs; a.num_obs = ll->dims[0]; a.num_actions = ll->dims[4]; a.deterministic = 1;
    for (int i = 0; i < 4; i++) {
        a.w[i] = ll->d_w[i]; a.b[i] = ll->d_b[i];
        W.wb[i] = reinterpret_cast<const bf16x8g *>(ll->d_wb[i]); W.bb[i] = ll->d_bb[i];
    }
}

}  // namespace lg
