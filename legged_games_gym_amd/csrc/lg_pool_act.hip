// lg_pool_act.hip -- k_pool_act (include/legged_dec_game_pool.h): the shared actor launch of the decentralised predator-prey game with the
// weights of a sampled role chosen per 32-env block from a pool of actors.  A translation unit of its own, reached through launch_pool_act
// (lg_pool_act.h), so that the code hipcc generates for the kernels of lg_dec_game.hip and lg_kernels.hip does not depend on it.
//
// The roles are dec_actor_role (lg_dec_game_act.h), the calls of wide_actor_body that k_dec_act makes: a block computes, bit for bit, what
// k_dec_act computes for it when launched with the block's member as the role's handle.  Only the addresses of the weight, bias and std
// operands differ.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define LG_POLICY_BLOCKS_ONLY      // lg_policy.h without its two non-template pack kernels (they belong to lg_learner.hip)
#include "lg_device.h"
#include "lg_policy.h"
#include "lg_pool_act.h"
#include "lg_dec_game_act.h"

namespace lg {

// The operands of a sampled role for workgroup `blk`: W as it stands in the kernel arguments, or with the nine pointers of the block's pool
// member.  blk comes from blockIdx alone, so the slot, the row address and the nine pointers are workgroup-uniform; the slot table and the
// pool's table are not written while the kernel runs, so they are read through the constant address space: scalar loads, the pointers stay
// in SGPRs as the kernel arguments of k_dec_act do.  The row is read from global memory -- a run-time index into the by-value arguments
// would copy them to scratch.  A slot outside [0, count) is clamped: a stale table must never index past the pool.
#define LG_CONST_AS __attribute__((address_space(4)))
LG_DEV PolicyWideArgs pool_role_args(const PolicyWideArgs &W, const DecPoolRole &R, const int blk) {
    PolicyWideArgs M = W;
    if (R.table) {
        const int slot = min(max(((const LG_CONST_AS int32_t *)R.block_slot)[blk], 0), R.count - 1);
        const LG_CONST_AS DecPoolEntry *m = (const LG_CONST_AS DecPoolEntry *)R.table + slot;
#pragma unroll
        for (int i = 0; i < 4; i++) { M.wb[i] = m->wb[i]; M.bb[i] = m->bb[i]; }
        M.base.std = m->std;
    }
    return M;
}

__global__ void __launch_bounds__(64 * LG_PW_WAVES) k_pool_act(const PoolActArgs G) {
    __shared__ bf16x8g xa[16][2][64], xb[32][2][64];               // as k_dec_act (96 KB), the same for all roles
    const DecActArgs &D = G.act;
    const int role = (int)blockIdx.x / D.blocks, blk = (int)blockIdx.x - role * D.blocks;      // every role has `blocks` workgroups, the low-level role the first
    if (role == 0) dec_actor_role<0>(D.ll, D, blk, xa, xb);
    else if (role == 1) dec_actor_role<1>(pool_role_args(D.prey, G.prey, blk), D, blk, xa, xb);
    else dec_actor_role<2>(pool_role_args(D.pred, G.pred, blk), D, blk, xa, xb);
}

int launch_pool_act(const PoolActArgs &G, void *stream) {
    hipLaunchKernelGGL(k_pool_act, dim3(3 * G.act.blocks), dim3(64 * LG_PW_WAVES), 0, (hipStream_t)stream, G);
    return (int)hipGetLastError();
}

}  // namespace lg
