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
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#define LG_POLICY_BLOCKS_ONLY      // lg_policy.h without its two non-template pack kernels
#include "lg_device.h"
#include "lg_policy.h"
#include "lg_host.h"               // struct lg_policy
#include "lg_dec_game_common.h"    // DecActAgent; include/legged_dec_game.h
#include "lg_dec_game_act.h"       // dec_command_epilogue<PREY>
#include "lg_recurrent.h"          // struct lg_lstm, lg_lstm_actor, LstmRole, LstmActorArgs, LG_LSTM_LD
#include "lg_lstm_cell_body.h"
#include "lg_lstm_actor_body.h"
#include "../../include/legged_dec_game_recurrent.h"

namespace lg {

// ------------------------------------------------------------------ k_dec_lstm_cell
struct DecLstmArgs {
    LstmRole role[4];              // predator actor / critic memory, prey actor / critic memory; only the present ones are filled
    const uint8_t *reset;
    int32_t num_envs, blocks;      // workgroups per present role
    uint32_t order, _pad;          // two bits per slot: the role of workgroups slot * blocks .. (slot + 1) * blocks - 1
};

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

static size_t cell_lds_bytes(const int ksteps) { return (size_t)2 * ksteps * LG_LSTM_LD * sizeof(float); }
static const int LSTM_MAX_KSTEPS = (LG_LSTM_MAX_IN + LG_LSTM_MAX_HIDDEN) / 2;

// ------------------------------------------------------------------ k_dec_game_lstm_act
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

__global__ void __launch_bounds__(64 * LG_PW_WAVES) k_dec_game_lstm_act(const DecGameLstmActArgs G) {
    // ONE dynamic block, carved per role (host: dec_game_lstm_lds_bytes):
    //   low-level role    bf16x8g xa[16][2][64], xb[32][2][64]                               96 KB, as k_policy_act_wide
    //   sampled roles     float xa[max_width][LG_LSTM_LD], xb[the same], ns[32][16], ms[32][16]
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

static size_t dec_game_lstm_lds_bytes(const int max_width) {
    const size_t hl = ((size_t)2 * max_width * LG_LSTM_LD + 32 * 16 + 32 * 16) * sizeof(float), ll = 98304;
    return hl > ll ? hl : ll;
}

static thread_local char g_error[512] = "";
static int refuse(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}

// above the 64 KB a kernel gets without asking: raised once per device, at the first call (outside any capture)
static hipError_t raise_lds_limit(const void *kernel, const size_t bytes, bool (&raised)[64]) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !raised[dev]) {
        e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) raised[dev] = true;
    }
    return hipSuccess;
}

static void fill_lstm_actor_args(LstmActorArgs &A, const lg_lstm_actor *a, const float *h, float *sample, float *mean, const int num_envs,
                                 const uint64_t seed, const int64_t step, const int64_t *step_counter, const int deterministic) {   // as lg_lstm_actor_act
    A.h = h; A.p = a->d_p; A.std = a->d_std; A.actions = sample; A.mean = mean; A.step_counter = step_counter;
    A.seed = seed; A.step = step; A.num_envs = num_envs; A.deterministic = deterministic; A.max_width = a->max_width;
    for (int i = 0; i < 5; i++) { A.dims[i] = a->dims[i]; A.pad[i] = a->pad[i]; }
    for (int i = 0; i < 4; i++) { A.w_off[i] = (uint32_t)a->w_off[i]; A.b_off[i] = (uint32_t)a->b_off[i]; }
}

}  // namespace lg

#undef HIP_TRY                     // lg_host.h's reports through the main library's lg::fail
#define HIP_TRY(x) do { hipError_t _e = (x); if (_e != hipSuccess) return lg::refuse(-10, "%s: HIP error: %s", who, hipGetErrorString(_e)); } while (0)

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
        K.x = R.x; K.h_in = R.h_in; K.c_in = R.c_in; K.h_out = R.h_out; K.c_out = R.c_out;
        K.wp = R.l->d_wp; K.bp = R.l->d_bp; K.num_in = R.l->num_in; K.hidden = R.l->hidden; K.ksteps = R.l->ksteps;
        if (K.hidden > hidden) hidden = K.hidden;
        if (K.ksteps > ksteps) ksteps = K.ksteps;
        A.order |= (uint32_t)r << (2 * slot++);
    }
    if (hidden < 32 || hidden > LG_LSTM_MAX_HIDDEN || hidden % 32 || ksteps < 1 || ksteps > lg::LSTM_MAX_KSTEPS)
        return lg::refuse(-2, "%s: a handle's shape is outside what lg_lstm_create makes", who);
    static bool raised[64] = {};
    HIP_TRY(lg::raise_lds_limit((const void *)lg::k_dec_lstm_cell, lg::cell_lds_bytes(lg::LSTM_MAX_KSTEPS), raised));
    A.reset = reset;
    A.num_envs = num_envs;
    A.blocks = (num_envs + LG_LSTM_BLOCK_ENVS - 1) / LG_LSTM_BLOCK_ENVS;
    hipLaunchKernelGGL(lg::k_dec_lstm_cell, dim3(present * A.blocks), dim3(2 * hidden), lg::cell_lds_bytes(ksteps), (hipStream_t)stream, A);
    HIP_TRY(hipGetLastError());
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
    HIP_TRY(lg::raise_lds_limit((const void *)lg::k_dec_game_lstm_act, lg::dec_game_lstm_lds_bytes(512), raised));

    lg::DecGameLstmActArgs g = {};
    lg::PolicyArgs &a = g.ll.base;                                 // what fill_policy_args / fill_wide_operands do for lg_policy_act(ll, deterministic = 1)
    a.obs = ll_obs; a.actions = ll_actions; a.mean = nullptr; a.std = ll->d_std; a.step_counter = step_counter; a.step = step; a.seed = seed_prey;
    a.num_envs = P->num_envs; a.num_obs = ll->dims[0]; a.num_actions = ll->dims[4]; a.deterministic = 1;
    for (int i = 0; i < 4; i++) {
        a.w[i] = ll->d_w[i]; a.b[i] = ll->d_b[i];
        g.ll.wb[i] = reinterpret_cast<const lg::bf16x8g *>(ll->d_wb[i]); g.ll.bb[i] = ll->d_bb[i];
    }
    lg::fill_lstm_actor_args(g.prey, prey, h_prey, oy.sample, mean_prey, P->num_envs, seed_prey, step, step_counter, deterministic_prey);
    lg::fill_lstm_actor_args(g.pred, pred, h_pred, op.sample, mean_pred, P->num_envs, seed_pred, step, step_counter, deterministic_pred);
    g.P = *P;
    g.a_prey = {B->command_prey, oy.sigma, oy.log_prob, oy.obs_copy};
    g.a_pred = {B->command_pred, op.sigma, op.log_prob, op.obs_copy};
    g.prey_obs = prey_obs; g.pred_obs = pred_obs; g.ll_commands = B->ll_commands;
    g.blocks = (P->num_envs + LG_PW_ENVS - 1) / LG_PW_ENVS;
    const int width = pred->max_width > prey->max_width ? pred->max_width : prey->max_width;
    hipLaunchKernelGGL(lg::k_dec_game_lstm_act, dim3(3 * g.blocks), dim3(64 * LG_PW_WAVES), lg::dec_game_lstm_lds_bytes(width), (hipStream_t)stream, g);
    HIP_TRY(hipGetLastError());
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
