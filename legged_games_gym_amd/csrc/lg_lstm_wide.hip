// lg_lstm_wide.hip -- k_lstm_wide_cell / k_lstm_wide_actor, their pack kernels and entry points (include/legged_recurrent_wide.h): the two
// LSTM memories of a recurrent policy with up to 512 units advanced by one rollout step in one launch, and the actor MLP behind such a
// memory.  The only translation unit of liblegged_lstm_wide.so: it links against nothing of the main library and owns its handles.
//
// The cell splits a memory's units over workgroups, not over more waves of one: a workgroup is 32 env rows x one unit group of up to 256
// units (8 waves).  Every workgroup stages the whole [x | h_in] block of its rows (stage_xh), then wave w of group g runs lg_lstm_cell_body.h's
// k-ordered chain (lstm_units) for units 256 g + 32 w ..: the same products in the same order from the same packed operands
// (lg_recurrent.h), the same epilogue.  h_out never aliases h_in, so the groups need no exchange.  What is this unit's own: all waves of a
// workgroup stage, a wave's unit group index, and the surplus-wave rule.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lg_device.h"             // rand4, f32x16, LG_DEV
#include "lg_recurrent.h"          // LstmRole, LstmActorArgs, LG_LSTM_LD: operand layout and lane maps
#include "lg_lstm_actor_body.h"    // the actor MLP chain, unchanged
#include "lg_lstm_cell_body.h"     // stage_xh, lstm_units, lstm_pack_body: the cell's bodies, shared
#include "lg_lib_error.h"          // g_error, refuse, HIP_TRY
#include "lg_memory_host.h"        // create / load_device / destroy / act of the handles, written once for the three cell libraries
#include "../../include/legged_recurrent_wide.h"

#define LG_LSTM_WIDE_GROUP_WAVES (LG_LSTM_WIDE_GROUP_UNITS / 32)
#define LG_LSTM_WIDE_ACTOR_WAVES 8

struct lg_lstm_wide {
    int32_t num_in, hidden, ksteps, device;
    float  *d_wp, *d_bp;
};

struct lg_lstm_wide_actor {        // as lg_lstm_actor (lg_recurrent.h), dims[0] up to 512
    int32_t dims[5], pad[5];
    int32_t device, max_width;
    size_t  w_off[4], b_off[4];
    float  *d_p, *d_std;
};

namespace lg {

struct LstmWideArgs {
    LstmRole role[2];              // actor memory, critic memory
    const uint8_t *reset;
    int32_t num_envs, blocks;      // 32-row blocks per unit group
    int32_t first_role, first_wgs; // role of workgroups 0 .. first_wgs - 1 (blocks x its unit groups); the other, when present, follows
};

// k_lstm_pack's layout (lg_recurrent.hip): [w_ih | w_hh] -> wp, b_ih + b_hh -> bp.  One thread per float4 of the packed layout.
__global__ void __launch_bounds__(256) k_lstm_wide_pack(const float *__restrict__ w_ih, const float *__restrict__ w_hh, const float *__restrict__ b_ih,
                                                        const float *__restrict__ b_hh, float4 *__restrict__ wp, float4 *__restrict__ bp,
                                                        const int num_in, const int hidden, const int ksteps) {
    lstm_pack_body(w_ih, w_hh, b_ih, b_hh, wp, bp, num_in, hidden, ksteps);       // lg_lstm_cell_body.h
}

// One role's workgroup: env rows 32 blk .. 32 blk + 31, units 256 grp .. of the role's memory.  All waves of the workgroup stage (the
// launch is sized for the widest group of the widest role); a wave past the group's units then only meets the barrier.
__device__ __forceinline__ void lstm_wide_role(const LstmRole &R, const uint8_t *__restrict__ reset, const int num_envs, const int blk, const int grp,
                                               float *xs) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = (int)blockDim.x;
    const int H = R.hidden, env0 = 32 * blk;
    stage_xh(R.x, R.h_in, R.num_in, H, reset, num_envs, env0, tid, nthreads, xs);
    __syncthreads();
    const int gw = LG_LSTM_WIDE_GROUP_WAVES * grp + wave;                             // the wave's 32 units among the memory's
    if (wave >= LG_LSTM_WIDE_GROUP_WAVES || gw >= H / 32) return;
    lstm_units(R, reset, num_envs, env0, gw, lane, xs);
}

__global__ void __launch_bounds__(64 * LG_LSTM_WIDE_GROUP_WAVES) k_lstm_wide_cell(const LstmWideArgs A) {
    extern __shared__ float xs[];                                                 // [2 ksteps][LG_LSTM_LD]
    const int second = (int)blockIdx.x >= A.first_wgs;
    const int at = (int)blockIdx.x - (second ? A.first_wgs : 0);
    const int grp = at / A.blocks, blk = at - grp * A.blocks;                     // a group's row blocks are neighbours: they stream the same weights
    if ((second ? 1 : A.first_role) == 0) lstm_wide_role(A.role[0], A.reset, A.num_envs, blk, grp, xs);
    else lstm_wide_role(A.role[1], A.reset, A.num_envs, blk, grp, xs);
}

// k_lstm_actor_pack's layout (lg_recurrent.hip): one layer of the actor MLP, one thread per packed weight, then the padded bias.
__global__ void __launch_bounds__(256) k_lstm_wide_actor_pack(const float *__restrict__ w, const float *__restrict__ b, float *__restrict__ wp,
                                                              float *__restrict__ bp, const int in, const int out, const int out_pad) {
    lstm_actor_pack_body(w, b, wp, bp, in, out, out_pad);                          // lg_lstm_actor_body.h
}

__global__ void __launch_bounds__(64 * LG_LSTM_WIDE_ACTOR_WAVES) k_lstm_wide_actor(const LstmActorArgs A) {
    extern __shared__ float lds[];                    // two activation buffers [max_width][LG_LSTM_LD], then the noise [32][16]
    float *xa = lds, *xb = lds + (size_t)A.max_width * LG_LSTM_LD, *ns = xb + (size_t)A.max_width * LG_LSTM_LD;
    lstm_actor_body<LG_LSTM_WIDE_ACTOR_WAVES, 16>(A, (int)blockIdx.x, xa, xb, ns, LstmActorStores{});     // lg_lstm_actor_body.h
}

struct LstmWideMemory {            // lg_memory_host.h: the traits of lg_lstm_wide
    using Handle = lg_lstm_wide;
    static constexpr int GATES = 4, MAX_IN = LG_LSTM_WIDE_MAX_IN, MAX_HIDDEN = LG_LSTM_WIDE_MAX_HIDDEN;
    static const char *name() { return "lg_lstm_wide"; }
    static const char *hidden_note() { return " (one layer, LSTM only)"; }
    static const void *cell_kernel() { return (const void *)k_lstm_wide_cell; }        // 101 376 B of staged [x | h] at the largest shape
    template <class... Args> static void pack(const dim3 grid, hipStream_t stream, Args... args) { hipLaunchKernelGGL(k_lstm_wide_pack, grid, dim3(256), 0, stream, args...); }
    static int error(const int code, const char *msg) { return refuse(code, "%s", msg); }
};

struct LstmWideActor {             // lg_memory_host.h: the traits of lg_lstm_wide_actor
    using Handle = lg_lstm_wide_actor;
    static constexpr int MAX_HIDDEN = LG_LSTM_WIDE_MAX_HIDDEN;
    static const char *name() { return "lg_lstm_wide_actor"; }
    static const void *actor_kernel() { return (const void *)k_lstm_wide_actor; }
    template <class... Args> static void pack(const dim3 grid, hipStream_t stream, Args... args) { hipLaunchKernelGGL(k_lstm_wide_actor_pack, grid, dim3(256), 0, stream, args...); }
    static void act(const dim3 grid, const size_t lds, hipStream_t stream, const LstmActorArgs &A) {
        hipLaunchKernelGGL(k_lstm_wide_actor, grid, dim3(64 * LG_LSTM_WIDE_ACTOR_WAVES), lds, stream, A);
    }
    static int error(const int code, const char *msg) { return refuse(code, "%s", msg); }
};

}  // namespace lg

extern "C" {

int lg_lstm_wide_create(int32_t num_in, int32_t hidden, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                        int32_t device_id, lg_lstm_wide **out) {
    return lg::memory_create<lg::LstmWideMemory>(num_in, hidden, w_ih, w_hh, b_ih, b_hh, device_id, out);
}

int lg_lstm_wide_load_device(lg_lstm_wide *l, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, void *stream) {
    return lg::memory_load_device<lg::LstmWideMemory>(l, w_ih, w_hh, b_ih, b_hh, stream);
}

int lg_lstm_wide_destroy(lg_lstm_wide *l) { return lg::memory_destroy<lg::LstmWideMemory>(l); }

int lg_lstm_wide_step(const lg_lstm_wide *l_a, const lg_lstm_wide *l_c, const float *x_a, const float *x_c, const uint8_t *reset,
                      const float *h_in_a, const float *c_in_a, float *h_out_a, float *c_out_a,
                      const float *h_in_c, const float *c_in_c, float *h_out_c, float *c_out_c, int32_t num_envs, void *stream) {
    const int rc = lg::lstm_step_check<lg::LstmWideMemory>(l_a, l_c, x_a, x_c, h_in_a, c_in_a, h_out_a, c_out_a, h_in_c, c_in_c, h_out_c, c_out_c, num_envs);
    if (rc) return rc;
    lg::LstmWideArgs A = {};
    if (l_a) lg::fill_lstm_role(A.role[0], l_a, x_a, h_in_a, c_in_a, h_out_a, c_out_a);
    if (l_c) lg::fill_lstm_role(A.role[1], l_c, x_c, h_in_c, c_in_c, h_out_c, c_out_c);
    auto groups = [](const lg_lstm_wide *l) { return l ? (l->hidden + LG_LSTM_WIDE_GROUP_UNITS - 1) / LG_LSTM_WIDE_GROUP_UNITS : 0; };
    A.reset = reset;
    A.num_envs = num_envs;
    A.blocks = (num_envs + LG_LSTM_WIDE_BLOCK_ENVS - 1) / LG_LSTM_WIDE_BLOCK_ENVS;
    A.first_role = l_a ? 0 : 1;
    A.first_wgs = A.blocks * groups(l_a ? l_a : l_c);
    const int wgs = A.blocks * (groups(l_a) + groups(l_c));
    const int hidden = max(l_a ? l_a->hidden : 0, l_c ? l_c->hidden : 0), ksteps = max(l_a ? l_a->ksteps : 0, l_c ? l_c->ksteps : 0);
    const int waves = min(hidden / 32, LG_LSTM_WIDE_GROUP_WAVES);
    hipLaunchKernelGGL(lg::k_lstm_wide_cell, dim3(wgs), dim3(64 * waves), lg::cell_lds_bytes(ksteps), (hipStream_t)stream, A);
    HIP_TRY(hipGetLastError());
    return 0;
}

int lg_lstm_wide_actor_create(const int32_t dims[5], int32_t device_id, lg_lstm_wide_actor **out) {
    return lg::actor_create<lg::LstmWideActor>(dims, device_id, out);
}

int lg_lstm_wide_actor_load_device(lg_lstm_wide_actor *a, const float *const weights[4], const float *const biases[4], const float *std, void *stream) {
    return lg::actor_load_device<lg::LstmWideActor>(a, weights, biases, std, stream);
}

int lg_lstm_wide_actor_destroy(lg_lstm_wide_actor *a) { return lg::actor_destroy<lg::LstmWideActor>(a); }

int lg_lstm_wide_actor_act(const lg_lstm_wide_actor *a, const float *h, float *actions, float *mean, int32_t num_envs, uint64_t seed, int64_t step,
                           const int64_t *step_counter, int32_t deterministic, void *stream) {
    return lg::actor_act<lg::LstmWideActor>(a, h, actions, mean, num_envs, seed, step, step_counter, deterministic, stream);
}

const char *lg_lstm_wide_last_error(void) { return lg::g_error; }

}  // extern "C"
