// lg_dec_game_lstm_act.hip -- k_dec_lstm_cell / lg_dec_lstm_step and k_dec_game_lstm_act / lg_dec_game_lstm_act
// (include/legged_dec_game_recurrent.h): the policy stage of a decentralised game step with two recurrent agents in two launches.
//   k_dec_lstm_cell       up to four memories (predator actor / critic, prey actor / critic), workgroups split by role; a role is a call of
//                         lstm_cell_role (lg_lstm_cell_body.h), the call k_lstm_cell makes: the same bits
//   k_dec_game_lstm_act   k_dec_act (lg_dec_game.hip) with recurrent sampled roles:
//     low-level role      wide_actor_body<15, 16, 8, 4> (lg_policy.h), the call k_dec_act and k_policy_act_wide<15,16,8,4> make
//     prey / predator     lstm_actor_body<LG_PW_WAVES, 16> (lg_lstm_actor_body.h), the chain of k_lstm_actor on 8 waves with 16 k-steps of
//                         weights requested ahead (the same bits), on the agent's actor memory's h; the means go to LDS and one thread per
//                         env then calls dec_command_epilogue<PREY> (lg_dec_game_act.h), the epilogue of k_dec_act's sampled roles
// The only translation unit of liblegged_dec_game_recurrent.so: it links against nothing of the other libraries.  The layouts of the
// handles the main library created (lg_policy, lg_lstm_actor, lg_lstm) come from the headers both are compiled from; the kernel arguments
// are filled here (fill_policy_args / fill_wide_operands / fail of lg_host.h live in other units and are not called).
#include <hip/hip_runtime.h>
#include <stdint.h>

#define LG_POLICY_BLOCKS_ONLY      // lg_policy.h without its two non-template pack kernels
#include "lg_device.h"
#include "lg_policy.h"
#include "lg_host.h"               // struct lg_policy
#include "lg_dec_game_common.h"    // DecActAgent; include/legged_dec_game.h
#include "lg_dec_game_act.h"       // dec_command_epilogue<PREY>
#include "lg_recurrent.h"          // struct lg_lstm, lg_lstm_actor, LstmRole, LstmActorArgs, LG_LSTM_LD
#include "lg_lstm_cell_body.h"
#include "lg_lstm_actor_body.h"
#include "lg_lib_error.h"            // g_error, refuse, raise_lds_limit, HIP_TRY_WHO
#include "lg_memory_host.h"          // cell_lds_bytes, fill_lstm_role, fill_lstm_actor_args
#include "lg_dec_lstm_act.h"         // DecLstmArgs, DecGameLstmActArgs, dec_lstm_actor_role<PREY>, the host code that sizes and fills them
#include "../../include/legged_dec_game_recurrent.h"

namespace lg {

// ------------------------------------------------------------------ k_dec_lstm_cell
__global__ void __launch_bounds__(2 * LG_LSTM_MAX_HIDDEN) k_dec_lstm_cell(const DecLstmArgs A) {
    extern __shared__ float xs[];                                                 // [2 ksteps of the largest present role][LG_LSTM_LD]
    const int slot = (int)blockIdx.x / A.blocks, blk = (int)blockIdx.x - slot * A.blocks;
    switch ((A.order >> (2 * slot)) & 3u) {                                       // (a constant index each: the arguments stay where they are)
        case 0: lstm_cell_role(A.role[0], A.reset, A.num_envs, blk, xs); break;
        case 1: lstm_cell_role(A.role[1], A.reset, A.num_envs, blk, xs); break;
        case 2: lstm_cell_role(A.role[2], A.reset, A.num_envs, blk, xs); break;
        default: lstm_cell_role(A.role[3], A.reset, A.num_envs, blk, xs); break;
    }
}

// ------------------------------------------------------------------ k_dec_game_lstm_act
__global__ void __launch_bounds__(64 * LG_PW_WAVES) k_dec_game_lstm_act(const DecGameLstmActArgs G) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int role = (int)blockIdx.x / G.blocks, blk = (int)blockIdx.x - role * G.blocks;      // every role has `blocks` workgroups, the low-level role the first
    if (role == 0) {
        bf16x8g (*xa)[2][64] = reinterpret_cast<bf16x8g (*)[2][64]>(smem);
        wide_actor_body<15, 16, 8, 4>(G.ll, blk, xa, xa + 16, WideNoTap{}, WideActStores{});
    } else if (role == 1) {
        dec_lstm_actor_role<true>(G.prey, G.a_prey, G.prey_obs, G.P, G.ll_commands, blk, smem);
    } else {
        dec_lstm_actor_role<false>(G.pred, G.a_pred, G.pred_obs, G.P, G.ll_commands, blk, smem);
    }
}

}  // namespace lg

extern "C" {

int lg_dec_lstm_step(const lg_dec_lstm_role roles[4], const uint8_t *reset, int32_t num_envs, void *stream) {
    static const char *const who = "lg_dec_lstm_step";
    static const char *const names[4] = {"predator actor", "predator critic", "prey actor", "prey critic"};
    if (!roles) return lg::refuse(-1, "%s: null roles", who);
    int present = 0, hidden = 0, ksteps = 0, device = 0;
    for (int r = 0; r < 4; r++) {
        const lg_dec_lstm_role &R = roles[r];
        if (!R.l) continue;
        if (!R.x || !R.h_in || !R.c_in || !R.h_out || !R.c_out) return lg::refuse(-1, "%s: null buffer of the %s memory", who, names[r]);
        present++;
    }
    if (!present) return lg::refuse(-1, "%s: all four handles are null", who);
    if (num_envs < 1) return lg::refuse(-2, "%s: num_envs must be >= 1", who);
    lg::DecLstmArgs A = {};
    int slot = 0;
    for (int r = 0; r < 4; r++) {
        const lg_dec_lstm_role &R = roles[r];
        if (!R.l) continue;
        if (R.h_out == R.h_in || R.h_out == R.c_in || R.c_out == R.h_in || R.c_out == R.c_in || R.h_out == R.c_out)
            return lg::refuse(-2, "%s: h_out / c_out of the %s memory must not alias h_in / c_in (other workgroups read them as the K operand)", who, names[r]);
        if (slot && R.l->device != device) return lg::refuse(-2, "%s: the memories live on different devices", who);
        device = R.l->device;
        lg::LstmRole &K = A.role[r];
        lg::fill_lstm_role(K, R.l, R.x, R.h_in, R.c_in, R.h_out, R.c_out);
        if (K.hidden > hidden) hidden = K.hidden;
        if (K.ksteps > ksteps) ksteps = K.ksteps;
        A.order |= (uint32_t)r << (2 * slot++);
    }
    if (hidden < 32 || hidden > LG_LSTM_MAX_HIDDEN || hidden % 32 || ksteps < 1 || ksteps > lg::LSTM_MAX_KSTEPS)
        return lg::refuse(-2, "%s: a handle's shape is outside what lg_lstm_create makes", who);
    static bool raised[64] = {};
    HIP_TRY_WHO(lg::raise_lds_limit((const void *)lg::k_dec_lstm_cell, lg::cell_lds_bytes(lg::LSTM_MAX_KSTEPS), raised));
    A.reset = reset;
    A.num_envs = num_envs;
    A.blocks = (num_envs + LG_LSTM_BLOCK_ENVS - 1) / LG_LSTM_BLOCK_ENVS;
    hipLaunchKernelGGL(lg::k_dec_lstm_cell, dim3(present * A.blocks), dim3(2 * hidden), lg::cell_lds_bytes(ksteps), (hipStream_t)stream, A);
    HIP_TRY_WHO(hipGetLastError());
    return 0;
}

int lg_dec_game_lstm_act(const lg_lstm_actor *pred, const lg_lstm_actor *prey, lg_policy *ll, const lg_dec_game_params *P, const lg_dec_game_buffers *B,
                         const float *h_pred, const float *h_prey, const float *pred_obs, const float *prey_obs, const float *ll_obs, float *ll_actions,
                         float *mean_pred, float *mean_prey, uint64_t seed_pred, uint64_t seed_prey, int64_t step, const int64_t *step_counter,
                         int32_t deterministic_pred, int32_t deterministic_prey, const lg_dec_act_outputs *out_pred, const lg_dec_act_outputs *out_prey,
                         void *stream) {
    static const char *const who = "lg_dec_game_lstm_act";
    if (!pred || !prey || !ll || !P || !B || !h_pred || !h_prey || !ll_obs || !ll_actions || !mean_pred || !mean_prey)
        return lg::refuse(-1, "%s: null argument", who);
    if (!B->command_prey || !B->command_pred || !B->ll_commands) return lg::refuse(-1, "%s: null command_prey, command_pred or ll_commands in the buffers", who);
    const lg_dec_act_outputs none = {nullptr, nullptr, nullptr, nullptr};
    const lg_dec_act_outputs &op = out_pred ? *out_pred : none, &oy = out_prey ? *out_prey : none;
    if ((op.obs_copy && !pred_obs) || (oy.obs_copy && !prey_obs)) return lg::refuse(-1, "%s: null observations of an agent whose obs_copy is given", who);
    if (P->num_envs < 1) return lg::refuse(-2, "%s: num_envs must be >= 1", who);
    if (pred->dims[4] != LG_DEC_NUM_ACTIONS_PRED || prey->dims[4] != LG_DEC_NUM_ACTIONS_PREY || !(ll->wide && ll->tiles[0] == 15))
        return lg::refuse(-4, "%s is compiled for a two-action and a four-action recurrent actor next to the wide 235-512-256-128 low-level actor; "
                              "use lg_lstm_actor_act x 2 + lg_dec_game_pre + lg_policy_act", who);
    if (pred->max_width < 32 || pred->max_width > 512 || prey->max_width < 32 || prey->max_width > 512)
        return lg::refuse(-4, "%s: layer widths of the recurrent actors must be 32 .. 512", who);
    if (seed_pred == seed_prey) return lg::refuse(-2, "%s: seed_pred and seed_prey must differ (the sampled roles share their noise purposes)", who);

    static bool raised[64] = {};
    HIP_TRY_WHO(lg::raise_lds_limit((const void *)lg::k_dec_game_lstm_act, lg::dec_game_lstm_lds_bytes(512), raised));

    lg::DecGameLstmActArgs g = {};
    lg::fill_ll_role_args(g.ll, ll, ll_obs, ll_actions, P->num_envs, seed_prey, step, step_counter);
    lg::fill_lstm_actor_args(g.prey, prey, h_prey, oy.sample, mean_prey, P->num_envs, seed_prey, step, step_counter, deterministic_prey);
    lg::fill_lstm_actor_args(g.pred, pred, h_pred, op.sample, mean_pred, P->num_envs, seed_pred, step, step_counter, deterministic_pred);
    g.P = *P;
    g.a_prey = {B->command_prey, oy.sigma, oy.log_prob, oy.obs_copy};
    g.a_pred = {B->command_pred, op.sigma, op.log_prob, op.obs_copy};
    g.prey_obs = prey_obs; g.pred_obs = pred_obs; g.ll_commands = B->ll_commands;
    g.blocks = (P->num_envs + LG_PW_ENVS - 1) / LG_PW_ENVS;
    const int width = pred->max_width > prey->max_width ? pred->max_width : prey->max_width;
    hipLaunchKernelGGL(lg::k_dec_game_lstm_act, dim3(3 * g.blocks), dim3(64 * LG_PW_WAVES), lg::dec_game_lstm_lds_bytes(width), (hipStream_t)stream, g);
    HIP_TRY_WHO(hipGetLastError());
    return 0;
}

const char *lg_dec_game_recurrent_last_error(void) { return lg::g_error; }

int lg_dec_game_recurrent_sizeof(int which) {
    switch (which) {
        case 0: return (int)sizeof(lg_dec_game_params);
        case 1: return (int)sizeof(lg_dec_game_buffers);
        case 2: return (int)sizeof(lg_dec_act_outputs);
        case 3: return (int)sizeof(lg_policy);
        case 4: return (int)sizeof(lg_lstm_actor);
        case 5: return (int)sizeof(lg_lstm);
        case 6: return (int)sizeof(lg_dec_lstm_role);
        default: return -1;
    }
}

}  // extern "C"
