// lg_pool_act.h -- what lg_game_entry.hip (the C entry points of include/legged_dec_game_pool.h, in lg_dec_game_pool_entry.h) and lg_pool_act.hip
// (k_pool_act) share: one row of a pool's device table, the kernel's argument struct and its launcher.  Needs lg_policy.h and
// lg_dec_game_common.h.  The kernel is a translation unit of its own for the reason lg_dec_game.hip is one (lg_dec_game_common.h).
#pragma once
#include "lg_dec_game_common.h"
#include "../../include/legged_dec_game_pool.h"

static_assert(LG_DEC_POOL_BLOCK_ENVS == LG_PW_ENVS, "a block of the slot tables is the 32 envs of one workgroup of a role");

namespace lg {

// What a sampled role of k_dec_act takes from its lg_policy handle besides the shapes: the nine pointers of one pool member.  They are
// the handle's own buffers, which lg_policy_load_device repacks in place, so a row never goes stale while its member lives.
struct DecPoolEntry {
    const bf16x8g *wb[4];
    const float *bb[4];
    const float *std;
};

// One sampled role's pool.  table == nullptr: the role is not pooled and runs on the operands in DecActArgs, as in k_dec_act.
struct DecPoolRole {
    const DecPoolEntry *table;             // DEVICE [LG_DEC_POOL_MAX], global memory: indexed at run time, so NOT an array in the kernel arguments
    const int32_t *block_slot;             // DEVICE [blocks] member of each 32-env block; clamped to [0, count) in the kernel
    int32_t count, _pad;
};

struct PoolActArgs {
    DecActArgs act;                        // exactly the arguments of k_dec_act
    DecPoolRole prey, pred;
};
int launch_pool_act(const PoolActArgs &G, void *stream);      // returns the hipError_t of the launch

}  // namespace lg
