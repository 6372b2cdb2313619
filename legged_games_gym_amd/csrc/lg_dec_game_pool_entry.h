// lg_dec_game_pool_entry.h -- C entry points of the decentralised game's opponent pool (include/legged_dec_game_pool.h).  Host code only:
// the kernel lives in lg_pool_act.hip behind launch_pool_act (lg_pool_act.h).  An entry header of lg_game_entry.hip; includes what it
// uses.
#pragma once
#include <new>
#include "lg_dec_game.h"            // fail / HIP_TRY, lg_policy, fill_wide_operands, wide_precision (lg_host.h); dec_game_check, fill_dec_act_args
#include "lg_pool_act.h"

struct lg_dec_pool {
    lg::DecPoolEntry *d_table;     // [LG_DEC_POOL_MAX]; rows count .. MAX - 1 repeat row 0
    const lg_policy *first;        // member 0: the shapes and the f32 operands fill_policy_args wants (the kernel reads neither of a pooled role)
    int32_t count, role, device;
};

static bool dec_pool_shape_ok(const lg_policy *p, int role) {
    const int obs = role == 1 ? LG_DEC_NUM_OBS_PREY : LG_DEC_NUM_OBS_PRED, act = role == 1 ? LG_DEC_NUM_ACTIONS_PREY : LG_DEC_NUM_ACTIONS_PRED;
    return p->wide && p->dims[0] == obs && p->dims[4] == act;
}

extern "C" {

int lg_dec_pool_create(lg_policy *const *members, int32_t count, int32_t role, int32_t device, lg_dec_pool **out) {
    if (!members || !out) return lg::fail(-1, "null argument");
    if (count < 1 || count > LG_DEC_POOL_MAX) return lg::fail(-2, "lg_dec_pool_create: count must be 1 .. LG_DEC_POOL_MAX (16)");
    if (role != 1 && role != 2) return lg::fail(-2, "lg_dec_pool_create: role must be 1 (prey) or 2 (predator)");
    for (int i = 0; i < count; i++) {
        if (!members[i]) return lg::fail(-1, "lg_dec_pool_create: a member is null");
        if (!dec_pool_shape_ok(members[i], role)) return lg::fail(-4, "lg_dec_pool_create: a member is not a %s actor", role == 1 ? "16-512-256-128-4 prey" : "3-512-256-128-2 predator");
        if (members[i]->device != device) return lg::fail(-2, "lg_dec_pool_create: a member lives on another device");
    }
    lg::DecPoolEntry rows[LG_DEC_POOL_MAX];
    for (int i = 0; i < LG_DEC_POOL_MAX; i++) {
        const lg_policy *p = members[i < count ? i : 0];
        lg::fill_wide_operands(p, rows[i].wb, rows[i].bb);
        rows[i].std = p->d_std;
    }
    HIP_TRY(hipSetDevice(device));
    lg_dec_pool *pool = new (std::nothrow) lg_dec_pool();
    if (!pool) return lg::fail(-5, "out of host memory");
    pool->d_table = nullptr; pool->first = members[0]; pool->count = count; pool->role = role; pool->device = device;
    if (hipMalloc(&pool->d_table, sizeof rows) != hipSuccess || hipMemcpy(pool->d_table, rows, sizeof rows, hipMemcpyHostToDevice) != hipSuccess) {
        if (pool->d_table) (void)hipFree(pool->d_table);
        delete pool;
        return lg::fail(-10, "lg_dec_pool_create: the device table could not be allocated or copied");
    }
    *out = pool;
    return 0;
}

int lg_dec_pool_destroy(lg_dec_pool *pool) {
    if (!pool) return lg::fail(-1, "null argument");
    if (pool->d_table) (void)hipFree(pool->d_table);
    delete pool;
    return 0;
}

int lg_dec_pool_query(const lg_dec_pool *pool, lg_dec_pool_info *info) {
    if (!pool || !info) return lg::fail(-1, "null argument");
    info->count = pool->count; info->role = pool->role; info->device = pool->device; info->_pad = 0; info->table = pool->d_table;
    return 0;
}

int lg_dec_pool_act(lg_policy *pred, lg_policy *prey, lg_policy *ll, const lg_dec_pool *pool_pred, const int32_t *block_slot_pred, const lg_dec_pool *pool_prey,
                    const int32_t *block_slot_prey, const lg_dec_game_params *P, const lg_dec_game_buffers *B, const float *pred_obs, const float *prey_obs,
                    const float *ll_obs, float *ll_actions, float *mean_pred, float *mean_prey, uint64_t seed_pred, uint64_t seed_prey, int64_t step,
                    const int64_t *step_counter, int32_t deterministic_pred, int32_t deterministic_prey, const lg_dec_act_outputs *out_pred,
                    const lg_dec_act_outputs *out_prey, void *stream) {
    if (int rc = dec_game_check(P, B)) return rc;
    if ((!pred && !pool_pred) || (!prey && !pool_prey) || !ll || !pred_obs || !prey_obs || !ll_obs || !ll_actions || !mean_pred || !mean_prey) return lg::fail(-1, "null argument");
    if ((pool_pred && !block_slot_pred) || (pool_prey && !block_slot_prey)) return lg::fail(-1, "lg_dec_pool_act: a pool needs its block_slot table");
    if (!B->command_prey || !B->command_pred || !B->ll_commands) return lg::fail(-1, "lg_dec_pool_act needs command_prey, command_pred and ll_commands");
    if (seed_pred == seed_prey) return lg::fail(-2, "lg_dec_pool_act: seed_pred and seed_prey must differ (the sampled roles share their noise purposes)");
    const lg_policy *py = pool_prey ? pool_prey->first : prey, *pd = pool_pred ? pool_pred->first : pred;
    const bool prey_ok = pool_prey ? pool_prey->role == 1 : dec_pool_shape_ok(prey, 1);
    const bool pred_ok = pool_pred ? pool_pred->role == 2 : dec_pool_shape_ok(pred, 2);
    const bool ll_ok = ll->wide && ll->tiles[0] == 15;
    if (lg::wide_precision() != 1 || !prey_ok || !pred_ok || !ll_ok)
        return lg::fail(-4, "the pooled actor launch is compiled for the 3-512-256-128-2 / 16-512-256-128-4 / 235-512-256-128 triple at wide precision 1; use lg_policy_act per member + lg_dec_game_pre");
    lg::PoolActArgs a;
    fill_dec_act_args(a.act, pd, py, ll, P, B, pred_obs, prey_obs, ll_obs, ll_actions, mean_pred, mean_prey, seed_pred, seed_prey, step, step_counter,
                      deterministic_pred, deterministic_prey, out_pred, out_prey);
    a.prey = {pool_prey ? pool_prey->d_table : nullptr, pool_prey ? block_slot_prey : nullptr, pool_prey ? pool_prey->count : 0, 0};
    a.pred = {pool_pred ? pool_pred->d_table : nullptr, pool_pred ? block_slot_pred : nullptr, pool_pred ? pool_pred->count : 0, 0};
    HIP_TRY((hipError_t)lg::launch_pool_act(a, stream));
    return 0;
}

int lg_dec_pool_sizeof(int which) { return which == 0 ? (int)sizeof(lg_dec_pool_info) : -1; }

}  // extern "C"
