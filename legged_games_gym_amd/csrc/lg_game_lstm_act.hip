// lg_game_lstm_act.hip -- k_game_lstm_act and lg_game_lstm_act (include/legged_game_recurrent.h): both actors of a high-level game step
// in one launch when the high-level actor sits behind an LSTM memory.  It is k_prey_act (lg_game_act.h) with another high-level role:
//   low-level role    wide_actor_body<15, 16, 8, 4> (lg_policy.h), the call k_prey_act and k_policy_act_wide<15,16,8,4> make
//   high-level role   lstm_actor_body<LG_PW_WAVES, 16> (lg_lstm_actor_body.h), the chain of k_lstm_actor on 8 waves with 16 k-steps of weights
//                     requested ahead (the same bits), on the actor memory's h; the six means go to LDS and one thread per env then does
//                     what prey_command_epilogue does (lg_game_act.h)
// The only translation unit of liblegged_game_recurrent.so: it links against nothing of the main library.  The layouts of the handles
// that library created (lg_policy, lg_lstm_actor) come from the headers both are compiled from; the kernel arguments are filled here
// (fill_policy_args / fill_wide_operands / fail of lg_host.h live in other units and are not called).
#include <hip/hip_runtime.h>
#include <stdint.h>

#define LG_POLICY_BLOCKS_ONLY      // lg_policy.h without its two non-template pack kernels
#include "lg_device.h"
#include "lg_policy.h"
#include "lg_host.h"               // struct lg_policy
#include "lg_game_common.h"        // game_clip, game_wrap_to_pi; include/legged_game.h
#include "lg_recurrent.h"          // struct lg_lstm_actor, LstmActorArgs, LG_LSTM_LD
#include "lg_lstm_actor_body.h"
#include "lg_lib_error.h"          // g_error, refuse, raise_lds_limit, HIP_TRY_WHO
#include "lg_memory_host.h"        // fill_lstm_actor_args
#include "../../include/legged_game_recurrent.h"

namespace lg {

struct GameLstmActArgs {
    PolicyWideArgs ll;                     // low-level role: deterministic
    LstmActorArgs hl;                      // high-level role: hl.actions = the unclipped sample or null, hl.mean
    lg_game_params P;
    const float *hl_obs;                   // [N,19], read only for obs_copy
    float *command, *ll_commands;          // [N,6] clipped / wrapped command, [N,4] its first four columns (what k_game_pre writes)
    float *sigma, *log_prob, *obs_copy;    // optional, as PreyActArgs
    int32_t ll_blocks;                     // workgroups per role: the low-level role takes the first `ll_blocks`, the high-level role the rest
};

// last layer of the high-level role: the mean of action `unit` of row `row` into ms[32][16]
struct MeansToLds {
    float *ms;
    LG_DEV void operator()(const LstmActorArgs &, int, int row, int unit, float m, const float *) const { ms[row * 16 + unit] = m; }
};

// One thread per env: the stores of lg_lstm_actor_act, then exactly k_game_pre on the sample -- same expressions, contraction off -- and
// the optional sigma / log-prob of the UNCLIPPED sample, its terms added in prey_command_epilogue's order.
LG_DEV void lstm_command_epilogue(const GameLstmActArgs &G, const int env, const float *ms, const float *ns) {
#pragma clang fp contract(off)
    const LstmActorArgs &A = G.hl;
    const lg_game_params &P = G.P;
    float m[LG_GAME_NUM_ACTIONS], v[LG_GAME_NUM_ACTIONS], sg[LG_GAME_NUM_ACTIONS], lp[2] = {0.0f, 0.0f};
#pragma unroll
    for (int a = 0; a < LG_GAME_NUM_ACTIONS; a++) {
        m[a] = ms[a]; v[a] = m[a] + ns[a]; sg[a] = A.std[a];
        const float z = (v[a] - m[a]) / sg[a];
        lp[a >> 2] += -0.5f * z * z - __logf(sg[a]) - 0.918938533f;
    }
    const size_t row = (size_t)env * LG_GAME_NUM_ACTIONS;
#pragma unroll
    for (int a = 0; a < LG_GAME_NUM_ACTIONS; a++) {
        A.mean[row + a] = m[a];
        if (A.actions) A.actions[row + a] = v[a];
        if (G.sigma) G.sigma[row + a] = sg[a];
    }
    const float c0 = game_clip(v[0], P.cmd_lin_vel_x[0], P.cmd_lin_vel_x[1]);
    const float c1 = game_clip(v[1], P.cmd_lin_vel_y[0], P.cmd_lin_vel_y[1]);
    const float c2 = P.heading_command ? game_wrap_to_pi(v[2]) : v[2];
    const float c3 = v[3];
    float *c = G.command + row;
    c[0] = c0; c[1] = c1; c[2] = c2; c[3] = c3;
    c[4] = game_clip(v[4], P.predator_lin_vel_x[0], P.predator_lin_vel_x[1]);
    c[5] = game_clip(v[5], P.predator_lin_vel_y[0], P.predator_lin_vel_y[1]);
    float *ll = G.ll_commands + (size_t)env * 4;
    ll[0] = c0; ll[1] = c1; ll[2] = c2; ll[3] = c3;
    if (G.log_prob) G.log_prob[env] = lp[0] + lp[1];
}

__global__ void __launch_bounds__(64 * LG_PW_WAVES) k_game_lstm_act(const GameLstmActArgs G) {
    // ONE dynamic block, carved per role (host: game_lstm_lds_bytes):
    //   low-level role    bf16x8g xa[16][2][64], xb[32][2][64]                               96 KB, as k_policy_act_wide
    //   high-level role   float xa[max_width][LG_LSTM_LD], xb[the same], ns[32][16], ms[32][16]
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const bool first = (int)blockIdx.x < G.ll_blocks;              // both roles have ll_blocks workgroups, the low-level role the first
    const int blk = first ? (int)blockIdx.x : (int)blockIdx.x - G.ll_blocks;
    if (first) {
        bf16x8g (*xa)[2][64] = reinterpret_cast<bf16x8g (*)[2][64]>(smem);
        wide_actor_body<15, 16, 8, 4>(G.ll, blk, xa, xa + 16, WideNoTap{}, WideActStores{});
        return;
    }
    const LstmActorArgs &A = G.hl;
    float *xa = reinterpret_cast<float *>(smem), *xb = xa + (size_t)A.max_width * LG_LSTM_LD, *ns = xb + (size_t)A.max_width * LG_LSTM_LD, *ms = ns + 32 * 16;
    const int tid = (int)threadIdx.x, env0 = 32 * blk;
    if (G.obs_copy) {                                              // the observations the memories read, for the storage / the other ping-pong buffer
        for (int e = tid; e < 32 * LG_GAME_NUM_OBS; e += 64 * LG_PW_WAVES) {
            const size_t at = (size_t)env0 * LG_GAME_NUM_OBS + e;
            if (at < (size_t)A.num_envs * LG_GAME_NUM_OBS) G.obs_copy[at] = G.hl_obs[at];
        }
    }
    lstm_actor_body<LG_PW_WAVES, 16>(A, blk, xa, xb, ns, MeansToLds{ms});      // (ends in a barrier: ms and ns are complete)
    if (tid < 32 && env0 + tid < A.num_envs) lstm_command_epilogue(G, env0 + tid, ms + tid * 16, ns + tid * 16);
}

static size_t game_lstm_lds_bytes(const int max_width) {
    const size_t hl = ((size_t)2 * max_width * LG_LSTM_LD + 32 * 16 + 32 * 16) * sizeof(float), ll = 98304;
    return hl > ll ? hl : ll;
}

}  // namespace lg

extern "C" {

int lg_game_lstm_act(const lg_lstm_actor *hl, lg_policy *ll, const lg_game_params *P, const lg_game_buffers *B, const float *h, const float *hl_obs,
                     const float *ll_obs, float *ll_actions, float *mean, uint64_t seed, int64_t step, const int64_t *step_counter,
                     int32_t deterministic, float *sample, float *sigma, float *log_prob, float *obs_copy, void *stream) {
    static const char *const who = "lg_game_lstm_act";
    if (!hl || !ll || !P || !B || !h || !ll_obs || !ll_actions || !mean) return lg::refuse(-1, "lg_game_lstm_act: null argument");
    if (!B->command || !B->ll_commands) return lg::refuse(-1, "lg_game_lstm_act: null command or ll_commands in the buffers");
    if (obs_copy && !hl_obs) return lg::refuse(-1, "lg_game_lstm_act: null hl_obs with obs_copy given");
    if (P->num_envs < 1) return lg::refuse(-2, "lg_game_lstm_act: num_envs must be >= 1");
    if (hl->dims[4] != LG_GAME_NUM_ACTIONS || !(ll->wide && ll->tiles[0] == 15))
        return lg::refuse(-4, "lg_game_lstm_act is compiled for a six-action recurrent actor next to the wide 235-512-256-128 low-level actor; "
                              "use lg_lstm_actor_act + lg_game_pre + lg_policy_act");
    if (hl->max_width < 32 || hl->max_width > 512) return lg::refuse(-4, "lg_game_lstm_act: layer widths of the recurrent actor must be 32 .. 512");

    static bool raised[64] = {};
    HIP_TRY_WHO(lg::raise_lds_limit((const void *)lg::k_game_lstm_act, lg::game_lstm_lds_bytes(512), raised));

    lg::GameLstmActArgs g = {};
    lg::PolicyArgs &a = g.ll.base;                                 // what fill_policy_args / fill_wide_operands do for lg_policy_act(ll, deterministic = 1)
    a.obs = ll_obs; a.actions = ll_actions; a.mean = nullptr; a.std = ll->d_std; a.step_counter = step_counter; a.step = step; a.seed = seed;
    a.num_envs = P->num_envs; a.num_obs = ll->dims[0]; a.num_actions = ll->dims[4]; a.deterministic = 1;
    for (int i = 0; i < 4; i++) {
        a.w[i] = ll->d_w[i]; a.b[i] = ll->d_b[i];
        g.ll.wb[i] = reinterpret_cast<const lg::bf16x8g *>(ll->d_wb[i]); g.ll.bb[i] = ll->d_bb[i];
    }
    lg::fill_lstm_actor_args(g.hl, hl, h, sample, mean, P->num_envs, seed, step, step_counter, deterministic);
    g.P = *P; g.hl_obs = hl_obs; g.command = B->command; g.ll_commands = B->ll_commands;
    g.sigma = sigma; g.log_prob = log_prob; g.obs_copy = obs_copy;
    const int blocks = (P->num_envs + LG_PW_ENVS - 1) / LG_PW_ENVS;
    g.ll_blocks = blocks;
    hipLaunchKernelGGL(lg::k_game_lstm_act, dim3(2 * blocks), dim3(64 * LG_PW_WAVES), lg::game_lstm_lds_bytes(hl->max_width), (hipStream_t)stream, g);
    HIP_TRY_WHO(hipGetLastError());
    return 0;
}

const char *lg_game_recurrent_last_error(void) { return lg::g_error; }

int lg_game_recurrent_sizeof(int which) {
    switch (which) {
        case 0: return (int)sizeof(lg_game_params);
        case 1: return (int)sizeof(lg_game_buffers);
        case 2: return (int)sizeof(lg_policy);
        case 3: return (int)sizeof(lg_lstm_actor);
        default: return -1;
    }
}

}  // extern "C"
