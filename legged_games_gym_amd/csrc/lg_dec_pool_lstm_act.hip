// lg_dec_pool_lstm_act.hip -- k_dec_pool_lstm_cell / lg_dec_pool_lstm_step and k_dec_pool_lstm_act / lg_dec_pool_lstm_act
// (include/legged_dec_pool_recurrent.h): the recurrent policy stage of a decentralised game step with the weights of an agent's ACTOR
// memory and actor MLP chosen per 32-env block from a pool of members.
//   k_dec_pool_lstm_cell   k_dec_lstm_cell (lg_dec_game_lstm_act.hip): the same role split, each role a call of lstm_cell_role
//                          (lg_lstm_cell_body.h) on a local copy of its LstmRole, wp / bp replaced by the block's member when the role has a pool
//   k_dec_pool_lstm_act    k_dec_game_lstm_act: the low-level role unchanged, a sampled role dec_lstm_actor_role<PREY> (lg_dec_lstm_act.h) on
//                          an LstmActorArgs whose p / std are the block's member's
// A block therefore computes, bit for bit, what the plain launches compute for it with the block's member as the role's handle: only the
// addresses of the operands differ.
// The only translation unit of liblegged_dec_pool_recurrent.so: it links against nothing of the other libraries.  The layouts of the
// handles the main library created (lg_policy, lg_lstm_actor, lg_lstm) come from the headers both are compiled from.
#include <hip/hip_runtime.h>
#include <new>
#include <stdint.h>
#include <string.h>

#define LG_POLICY_BLOCKS_ONLY      // lg_policy.h without its two non-template pack kernels
#include "lg_device.h"
#include "lg_policy.h"
#include "lg_host.h"               // struct lg_policy
#include "lg_dec_game_common.h"    // DecActAgent; include/legged_dec_game.h
#include "lg_dec_game_act.h"       // dec_command_epilogue<PREY>
#include "lg_recurrent.h"          // struct lg_lstm, lg_lstm_actor, LstmRole, LstmActorArgs, LG_LSTM_LD
#include "lg_lstm_cell_body.h"
#include "lg_lstm_actor_body.h"
#include "lg_lib_error.h"          // g_error, refuse, raise_lds_limit, HIP_TRY_WHO
#include "lg_memory_host.h"        // cell_lds_bytes, fill_lstm_role, fill_lstm_actor_args
#include "lg_dec_lstm_act.h"       // DecLstmArgs, DecGameLstmActArgs, dec_lstm_actor_role<PREY>, the host code that sizes and fills them
#include "../../include/legged_dec_pool_recurrent.h"

namespace lg {

struct DecRPoolEntry { const float *wp, *bp, *p, *std; };          // a member: its actor memory's packed weights / bias, its actor MLP's parameters / std
struct DecRPoolRole {
    const DecRPoolEntry *table;    // null: the role has no pool
    const int32_t *block_slot;
    int32_t count, _pad;
};

}  // namespace lg

struct lg_dec_rpool {
    lg::DecRPoolEntry *d_table;    // [LG_DEC_POOL_MAX]; rows count .. MAX - 1 repeat row 0
    int32_t count, role, device;
    lg_lstm lstm;                  // member 0's shapes (the pointers are not read: a pooled role's come from the table)
    lg_lstm_actor actor;
};

namespace lg {

// The row of a pooled role for workgroup `blk`.  blk comes from blockIdx alone, so the slot, the row address and the pointers are
// workgroup-uniform; neither table is written while the kernel runs, so both are read through the constant address space: scalar loads,
// the pointers stay in SGPRs as the kernel arguments of the plain launches do.  The row is read from global memory -- a run-time index
// into the by-value arguments would copy them to scratch.  A slot outside [0, count) is clamped: a stale table must never index past the pool.
#define LG_CONST_AS __attribute__((address_space(4)))
LG_DEV const LG_CONST_AS DecRPoolEntry *rpool_member(const DecRPoolRole &R, const int blk) {
    const int slot = min(max(((const LG_CONST_AS int32_t *)R.block_slot)[blk], 0), R.count - 1);
    return (const LG_CONST_AS DecRPoolEntry *)R.table + slot;
}

// ------------------------------------------------------------------ k_dec_pool_lstm_cell
struct DecPoolLstmArgs {
    DecLstmArgs cell;
    DecRPoolRole pred, prey;       // of role[0] (predator actor memory) / role[2] (prey actor memory)
};

LG_DEV LstmRole pool_lstm_role(const LstmRole &R, const DecRPoolRole &P, const int blk) {
    LstmRole M = R;
    if (P.table) {
        const LG_CONST_AS DecRPoolEntry *m = rpool_member(P, blk);
        M.wp = m->wp; M.bp = m->bp;
    }
    return M;
}

__global__ void __launch_bounds__(2 * LG_LSTM_MAX_HIDDEN) k_dec_pool_lstm_cell(const DecPoolLstmArgs G) {
    extern __shared__ float xs[];                                                 // [2 ksteps of the largest present role][LG_LSTM_LD]
    const DecLstmArgs &A = G.cell;
    const int slot = (int)blockIdx.x / A.blocks, blk = (int)blockIdx.x - slot * A.blocks;
    switch ((A.order >> (2 * slot)) & 3u) {                                       // (a constant index each: the arguments stay where they are)
        case 0: lstm_cell_role(pool_lstm_role(A.role[0], G.pred, blk), A.reset, A.num_envs, blk, xs); break;
        case 1: lstm_cell_role(A.role[1], A.reset, A.num_envs, blk, xs); break;
        case 2: lstm_cell_role(pool_lstm_role(A.role[2], G.prey, blk), A.reset, A.num_envs, blk, xs); break;
        default: lstm_cell_role(A.role[3], A.reset, A.num_envs, blk, xs); break;
    }
}

// ------------------------------------------------------------------ k_dec_pool_lstm_act
struct DecPoolLstmActArgs {
    DecGameLstmActArgs act;
    DecRPoolRole prey, pred;
};

LG_DEV LstmActorArgs pool_actor_args(const LstmActorArgs &A, const DecRPoolRole &P, const int blk) {
    LstmActorArgs M = A;
    if (P.table) {
        const LG_CONST_AS DecRPoolEntry *m = rpool_member(P, blk);
        M.p = m->p; M.std = m->std;
    }
    return M;
}

__global__ void __launch_bounds__(64 * LG_PW_WAVES) k_dec_pool_lstm_act(const DecPoolLstmActArgs Q) {
    extern __shared__ __attribute__((aligned(16))) char smem[];                   // carved per role as in k_dec_game_lstm_act (dec_game_lstm_lds_bytes)
    const DecGameLstmActArgs &G = Q.act;
    const int role = (int)blockIdx.x / G.blocks, blk = (int)blockIdx.x - role * G.blocks;      // every role has `blocks` workgroups, the low-level role the first
    if (role == 0) {
        bf16x8g (*xa)[2][64] = reinterpret_cast<bf16x8g (*)[2][64]>(smem);
        wide_actor_body<15, 16, 8, 4>(G.ll, blk, xa, xa + 16, WideNoTap{}, WideActStores{});
    } else if (role == 1) {
        dec_lstm_actor_role<true>(pool_actor_args(G.prey, Q.prey, blk), G.a_prey, G.prey_obs, G.P, G.ll_commands, blk, smem);
    } else {
        dec_lstm_actor_role<false>(pool_actor_args(G.pred, Q.pred, blk), G.a_pred, G.pred_obs, G.P, G.ll_commands, blk, smem);
    }
}

static int role_inputs(int role) { return role == 1 ? LG_DEC_NUM_OBS_PREY : LG_DEC_NUM_OBS_PRED; }
static int role_actions(int role) { return role == 1 ? LG_DEC_NUM_ACTIONS_PREY : LG_DEC_NUM_ACTIONS_PRED; }

static bool same_shape(const lg_lstm *l, const lg_lstm_actor *a, const lg_lstm *l0, const lg_lstm_actor *a0) {
    return l->num_in == l0->num_in && l->hidden == l0->hidden && l->ksteps == l0->ksteps && a->max_width == a0->max_width
        && !memcmp(a->dims, a0->dims, sizeof a->dims) && !memcmp(a->pad, a0->pad, sizeof a->pad)
        && !memcmp(a->w_off, a0->w_off, sizeof a->w_off) && !memcmp(a->b_off, a0->b_off, sizeof a->b_off);
}

static DecRPoolRole pool_role(const lg_dec_rpool *pool, const int32_t *block_slot) {
    if (!pool) return {nullptr, nullptr, 0, 0};
    return {pool->d_table, block_slot, pool->count, 0};
}

}  // namespace lg

extern "C" {

int lg_dec_rpool_create(const lg_lstm *const *lstm_members, const lg_lstm_actor *const *actor_members, int32_t count, int32_t role, int32_t device,
                        lg_dec_rpool **out) {
    static const char *const who = "lg_dec_rpool_create";
    if (!lstm_members || !actor_members || !out) return lg::refuse(-1, "%s: null argument", who);
    if (count < 1 || count > LG_DEC_POOL_MAX) return lg::refuse(-2, "%s: count must be 1 .. LG_DEC_POOL_MAX (%d), got %d", who, LG_DEC_POOL_MAX, count);
    if (role != 1 && role != 2) return lg::refuse(-2, "%s: role must be 1 (prey) or 2 (predator), got %d", who, role);
    for (int i = 0; i < count; i++) {
        const lg_lstm *l = lstm_members[i];
        const lg_lstm_actor *a = actor_members[i];
        if (!l || !a) return lg::refuse(-1, "%s: member %d is null", who, i);
        if (l->device != device || a->device != device) return lg::refuse(-2, "%s: member %d lives on another device", who, i);
        if (l->num_in != lg::role_inputs(role) || a->dims[4] != lg::role_actions(role) || a->dims[0] != l->hidden)
            return lg::refuse(-4, "%s: member %d is not a %s: an actor memory of %d inputs and an actor of %d actions on its units", who, i,
                              role == 1 ? "prey" : "predator", lg::role_inputs(role), lg::role_actions(role));
        if (!lg::same_shape(l, a, lstm_members[0], actor_members[0])) return lg::refuse(-4, "%s: the shape of member %d differs from member 0's", who, i);
    }
    lg::DecRPoolEntry rows[LG_DEC_POOL_MAX];
    for (int i = 0; i < LG_DEC_POOL_MAX; i++) {
        const int m = i < count ? i : 0;
        rows[i] = {lstm_members[m]->d_wp, lstm_members[m]->d_bp, actor_members[m]->d_p, actor_members[m]->d_std};
    }
    HIP_TRY_WHO(hipSetDevice(device));
    lg_dec_rpool *pool = new (std::nothrow) lg_dec_rpool();
    if (!pool) return lg::refuse(-5, "%s: out of host memory", who);
    pool->d_table = nullptr; pool->count = count; pool->role = role; pool->device = device;
    pool->lstm = *lstm_members[0]; pool->actor = *actor_members[0];
    pool->lstm.d_wp = pool->lstm.d_bp = nullptr; pool->actor.d_p = pool->actor.d_std = nullptr;
    if (hipMalloc(&pool->d_table, sizeof rows) != hipSuccess || hipMemcpy(pool->d_table, rows, sizeof rows, hipMemcpyHostToDevice) != hipSuccess) {
        if (pool->d_table) (void)hipFree(pool->d_table);
        delete pool;
        return lg::refuse(-10, "%s: the device table could not be allocated or copied", who);
    }
    *out = pool;
    return 0;
}

int lg_dec_rpool_destroy(lg_dec_rpool *pool) {
    if (!pool) return lg::refuse(-1, "lg_dec_rpool_destroy: null argument");
    if (pool->d_table) (void)hipFree(pool->d_table);
    delete pool;
    return 0;
}

int lg_dec_rpool_query(const lg_dec_rpool *pool, lg_dec_rpool_info *info) {
    if (!pool || !info) return lg::refuse(-1, "lg_dec_rpool_query: null argument");
    info->count = pool->count; info->role = pool->role; info->device = pool->device;
    info->num_in = pool->lstm.num_in; info->hidden = pool->lstm.hidden; info->ksteps = pool->lstm.ksteps;
    for (int i = 0; i < 5; i++) info->dims[i] = pool->actor.dims[i];
    info->max_width = pool->actor.max_width;
    info->table = pool->d_table;
    return 0;
}

int lg_dec_pool_lstm_step(const lg_dec_lstm_role roles[4], const lg_dec_rpool *pool_pred, const int32_t *block_slot_pred, const lg_dec_rpool *pool_prey,
                          const int32_t *block_slot_prey, const uint8_t *reset, int32_t num_envs, void *stream) {
    static const char *const who = "lg_dec_pool_lstm_step";
    static const char *const names[4] = {"predator actor", "predator critic", "prey actor", "prey critic"};
    if (!roles) return lg::refuse(-1, "%s: null roles", who);
    if ((pool_pred && !block_slot_pred) || (pool_prey && !block_slot_prey)) return lg::refuse(-1, "%s: a pool needs its block_slot table", who);
    const lg_dec_rpool *const pools[4] = {pool_pred, nullptr, pool_prey, nullptr};
    const lg_lstm *shape[4];                                       // a pooled role's shape comes from the pool, its handle is ignored
    int present = 0, hidden = 0, ksteps = 0, device = 0;
    for (int r = 0; r < 4; r++) {
        const lg_dec_lstm_role &R = roles[r];
        shape[r] = pools[r] ? &pools[r]->lstm : R.l;
        if (!shape[r]) continue;
        if (!R.x || !R.h_in || !R.c_in || !R.h_out || !R.c_out) return lg::refuse(-1, "%s: null buffer of the %s memory", who, names[r]);
        present++;
    }
    if (!present) return lg::refuse(-1, "%s: all four handles are null and there is no pool", who);
    if (num_envs < 1) return lg::refuse(-2, "%s: num_envs must be >= 1", who);
    if ((pool_pred && pool_pred->role != 2) || (pool_prey && pool_prey->role != 1))
        return lg::refuse(-4, "%s: a pool was created for the other role", who);
    lg::DecPoolLstmArgs G = {};
    lg::DecLstmArgs &A = G.cell;
    int slot = 0;
    for (int r = 0; r < 4; r++) {
        const lg_dec_lstm_role &R = roles[r];
        const lg_lstm *l = shape[r];
        if (!l) continue;
        if (R.h_out == R.h_in || R.h_out == R.c_in || R.c_out == R.h_in || R.c_out == R.c_in || R.h_out == R.c_out)
            return lg::refuse(-2, "%s: h_out / c_out of the %s memory must not alias h_in / c_in (other workgroups read them as the K operand)", who, names[r]);
        const int dev = pools[r] ? pools[r]->device : l->device;
        if (slot && dev != device) return lg::refuse(-2, "%s: the memories and pools live on different devices", who);
        device = dev;
        lg::LstmRole &K = A.role[r];
        lg::fill_lstm_role(K, l, R.x, R.h_in, R.c_in, R.h_out, R.c_out);             // (wp, bp null for a pooled role: the kernel takes the member's)
        if (K.hidden > hidden) hidden = K.hidden;
        if (K.ksteps > ksteps) ksteps = K.ksteps;
        A.order |= (uint32_t)r << (2 * slot++);
    }
    if (hidden < 32 || hidden > LG_LSTM_MAX_HIDDEN || hidden % 32 || ksteps < 1 || ksteps > lg::LSTM_MAX_KSTEPS)
        return lg::refuse(-2, "%s: a handle's shape is outside what lg_lstm_create makes", who);
    static bool raised[64] = {};
    HIP_TRY_WHO(lg::raise_lds_limit((const void *)lg::k_dec_pool_lstm_cell, lg::cell_lds_bytes(lg::LSTM_MAX_KSTEPS), raised));
    A.reset = reset;
    A.num_envs = num_envs;
    A.blocks = (num_envs + LG_LSTM_BLOCK_ENVS - 1) / LG_LSTM_BLOCK_ENVS;
    G.pred = lg::pool_role(pool_pred, block_slot_pred);
    G.prey = lg::pool_role(pool_prey, block_slot_prey);
    hipLaunchKernelGGL(lg::k_dec_pool_lstm_cell, dim3(present * A.blocks), dim3(2 * hidden), lg::cell_lds_bytes(ksteps), (hipStream_t)stream, G);
    HIP_TRY_WHO(hipGetLastError());
    return 0;
}

int lg_dec_pool_lstm_act(const lg_lstm_actor *pred, const lg_lstm_actor *prey, lg_policy *ll, const lg_dec_rpool *pool_pred, const int32_t *block_slot_pred,
                         const lg_dec_rpool *pool_prey, const int32_t *block_slot_prey, const lg_dec_game_params *P, const lg_dec_game_buffers *B,
                         const float *h_pred, const float *h_prey, const float *pred_obs, const float *prey_obs, const float *ll_obs, float *ll_actions,
                         float *mean_pred, float *mean_prey, uint64_t seed_pred, uint64_t seed_prey, int64_t step, const int64_t *step_counter,
                         int32_t deterministic_pred, int32_t deterministic_prey, const lg_dec_act_outputs *out_pred, const lg_dec_act_outputs *out_prey,
                         void *stream) {
    static const char *const who = "lg_dec_pool_lstm_act";
    if ((!pred && !pool_pred) || (!prey && !pool_prey) || !ll || !P || !B || !h_pred || !h_prey || !ll_obs || !ll_actions || !mean_pred || !mean_prey)
        return lg::refuse(-1, "%s: null argument", who);
    if ((pool_pred && !block_slot_pred) || (pool_prey && !block_slot_prey)) return lg::refuse(-1, "%s: a pool needs its block_slot table", who);
    if (!B->command_prey || !B->command_pred || !B->ll_commands) return lg::refuse(-1, "%s: null command_prey, command_pred or ll_commands in the buffers", who);
    const lg_dec_act_outputs none = {nullptr, nullptr, nullptr, nullptr};
    const lg_dec_act_outputs &op = out_pred ? *out_pred : none, &oy = out_prey ? *out_prey : none;
    if ((op.obs_copy && !pred_obs) || (oy.obs_copy && !prey_obs)) return lg::refuse(-1, "%s: null observations of an agent whose obs_copy is given", who);
    if (P->num_envs < 1) return lg::refuse(-2, "%s: num_envs must be >= 1", who);
    if ((pool_pred && pool_pred->role != 2) || (pool_prey && pool_prey->role != 1))
        return lg::refuse(-4, "%s: a pool was created for the other role; use lg_lstm_actor_act per member + lg_dec_game_pre + lg_policy_act", who);
    const lg_lstm_actor *pd = pool_pred ? &pool_pred->actor : pred, *py = pool_prey ? &pool_prey->actor : prey;      // a pooled role's shape comes from the pool
    if (pd->dims[4] != LG_DEC_NUM_ACTIONS_PRED || py->dims[4] != LG_DEC_NUM_ACTIONS_PREY || !(ll->wide && ll->tiles[0] == 15))
        return lg::refuse(-4, "%s is compiled for a two-action and a four-action recurrent actor next to the wide 235-512-256-128 low-level actor; "
                              "use lg_lstm_actor_act per member + lg_dec_game_pre + lg_policy_act", who);
    if (pd->max_width < 32 || pd->max_width > 512 || py->max_width < 32 || py->max_width > 512)
        return lg::refuse(-4, "%s: layer widths of the recurrent actors must be 32 .. 512", who);
    if (seed_pred == seed_prey) return lg::refuse(-2, "%s: seed_pred and seed_prey must differ (the sampled roles share their noise purposes)", who);

    static bool raised[64] = {};
    HIP_TRY_WHO(lg::raise_lds_limit((const void *)lg::k_dec_pool_lstm_act, lg::dec_game_lstm_lds_bytes(512), raised));

    lg::DecPoolLstmActArgs q = {};
    lg::DecGameLstmActArgs &g = q.act;
    lg::fill_ll_role_args(g.ll, ll, ll_obs, ll_actions, P->num_envs, seed_prey, step, step_counter);
    lg::fill_lstm_actor_args(g.prey, py, h_prey, oy.sample, mean_prey, P->num_envs, seed_prey, step, step_counter, deterministic_prey);
    lg::fill_lstm_actor_args(g.pred, pd, h_pred, op.sample, mean_pred, P->num_envs, seed_pred, step, step_counter, deterministic_pred);
    g.P = *P;
    g.a_prey = {B->command_prey, oy.sigma, oy.log_prob, oy.obs_copy};
    g.a_pred = {B->command_pred, op.sigma, op.log_prob, op.obs_copy};
    g.prey_obs = prey_obs; g.pred_obs = pred_obs; g.ll_commands = B->ll_commands;
    g.blocks = (P->num_envs + LG_PW_ENVS - 1) / LG_PW_ENVS;
    q.prey = lg::pool_role(pool_prey, block_slot_prey);
    q.pred = lg::pool_role(pool_pred, block_slot_pred);
    const int width = pd->max_width > py->max_width ? pd->max_width : py->max_width;
    hipLaunchKernelGGL(lg::k_dec_pool_lstm_act, dim3(3 * g.blocks), dim3(64 * LG_PW_WAVES), lg::dec_game_lstm_lds_bytes(width), (hipStream_t)stream, q);
    HIP_TRY_WHO(hipGetLastError());
    return 0;
}

const char *lg_dec_pool_recurrent_last_error(void) { return lg::g_error; }

int lg_dec_pool_recurrent_sizeof(int which) {
    switch (which) {
        case 0: return (int)sizeof(lg_dec_game_params);
        case 1: return (int)sizeof(lg_dec_game_buffers);
        case 2: return (int)sizeof(lg_dec_act_outputs);
        case 3: return (int)sizeof(lg_policy);
        case 4: return (int)sizeof(lg_lstm_actor);
        case 5: return (int)sizeof(lg_lstm);
        case 6: return (int)sizeof(lg_dec_lstm_role);
        case 7: return (int)sizeof(lg_dec_rpool_info);
        default: return -1;
    }
}

}  // extern "C"
