// lg_recurrent.hip -- k_lstm_cell / k_lstm_pack and their entry points (include/legged_recurrent.h): the two LSTM memories of a recurrent
// policy advanced by one rollout step in one launch.  Operand layout and lane maps: lg_recurrent.h.  A translation unit of its own: the
// code hipcc generates for the other units' kernels does not depend on it.  The kernels' bodies are the shared ones of lg_lstm_cell_body.h
// and lg_lstm_actor_body.h, the handles' lifecycle is lg_memory_host.h's: this unit holds the kernels' names, the traits and lg_lstm_step.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lg_device.h"             // rand4: the Philox stream of the actor kernels
#include "lg_recurrent.h"
#include "lg_lstm_actor_body.h"      // the actor MLP of k_lstm_actor, shared with the game layer's recurrent actor launch
#include "lg_lstm_cell_body.h"       // the cell of k_lstm_cell, shared with the cell launch of the decentralised game
#include "../../include/legged_recurrent.h"
#include "lg_memory_host.h"          // create / load_device / destroy / act of the handles, written once for the three cell libraries

#define HIP_TRY(x) do { hipError_t _e = (x); if (_e != hipSuccess) return lg::fail(-10, "HIP error: %s", hipGetErrorString(_e)); } while (0)

namespace lg {


// [w_ih | w_hh] (torch.nn.LSTM layout, gate order i, f, g, o) -> wp, b_ih + b_hh -> bp.  One thread per float4 of the packed layout.
__global__ void __launch_bounds__(256) k_lstm_pack(const float *__restrict__ w_ih, const float *__restrict__ w_hh, const float *__restrict__ b_ih,
                                                   const float *__restrict__ b_hh, float4 *__restrict__ wp, float4 *__restrict__ bp,
                                                   const int num_in, const int hidden, const int ksteps) {
    lstm_pack_body(w_ih, w_hh, b_ih, b_hh, wp, bp, num_in, hidden, ksteps);       // lg_lstm_cell_body.h
}

__global__ void __launch_bounds__(2 * LG_LSTM_MAX_HIDDEN) k_lstm_cell(const LstmArgs A) {
    extern __shared__ float xs[];                                                 // [2 ksteps][LG_LSTM_LD]
    const int second = (int)blockIdx.x >= A.blocks;
    const int blk = (int)blockIdx.x - (second ? A.blocks : 0);
    if ((second ? 1 : A.first_role) == 0) lstm_cell_role(A.role[0], A.reset, A.num_envs, blk, xs);
    else lstm_cell_role(A.role[1], A.reset, A.num_envs, blk, xs);
}


// One layer of the actor MLP into the packed layout; one thread per packed weight, then the padded bias.
__global__ void __launch_bounds__(256) k_lstm_actor_pack(const float *__restrict__ w, const float *__restrict__ b, float *__restrict__ wp,
                                                         float *__restrict__ bp, const int in, const int out, const int out_pad) {
    lstm_actor_pack_body(w, b, wp, bp, in, out, out_pad);                          // lg_lstm_actor_body.h
}

__global__ void __launch_bounds__(64 * LG_LSTM_ACTOR_WAVES) k_lstm_actor(const LstmActorArgs A) {
    extern __shared__ float lds[];                    // two activation buffers [max_width][LG_LSTM_LD], then the noise [32][16]
    float *xa = lds, *xb = lds + (size_t)A.max_width * LG_LSTM_LD, *ns = xb + (size_t)A.max_width * LG_LSTM_LD;
    lstm_actor_body<LG_LSTM_ACTOR_WAVES, 4>(A, (int)blockIdx.x, xa, xb, ns, LstmActorStores{});      // lg_lstm_actor_body.h
}

struct LstmMemory {                // lg_memory_host.h: the traits of lg_lstm
    using Handle = lg_lstm;
    static constexpr int GATES = 4, MAX_IN = LG_LSTM_MAX_IN, MAX_HIDDEN = LG_LSTM_MAX_HIDDEN;
    static const char *name() { return "lg_lstm"; }
    static const char *hidden_note() { return " (one layer, LSTM only)"; }
    static const void *cell_kernel() { return (const void *)k_lstm_cell; }
    template <class... Args> static void pack(const dim3 grid, hipStream_t stream, Args... args) { hipLaunchKernelGGL(k_lstm_pack, grid, dim3(256), 0, stream, args...); }
    static int error(const int code, const char *msg) { return fail(code, "%s", msg); }
};

struct LstmActor {                 // lg_memory_host.h: the traits of lg_lstm_actor
    using Handle = lg_lstm_actor;
    static constexpr int MAX_HIDDEN = LG_LSTM_MAX_HIDDEN;
    static const char *name() { return "lg_lstm_actor"; }
    static const void *actor_kernel() { return (const void *)k_lstm_actor; }
    template <class... Args> static void pack(const dim3 grid, hipStream_t stream, Args... args) { hipLaunchKernelGGL(k_lstm_actor_pack, grid, dim3(256), 0, stream, args...); }
    static void act(const dim3 grid, const size_t lds, hipStream_t stream, const LstmActorArgs &A) {
        hipLaunchKernelGGL(k_lstm_actor, grid, dim3(64 * LG_LSTM_ACTOR_WAVES), lds, stream, A);
    }
    static int error(const int code, const char *msg) { return fail(code, "%s", msg); }
};

}  // namespace lg

extern "C" {

int lg_lstm_create(int32_t num_in, int32_t hidden, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                   int32_t device_id, lg_lstm **out) {
    return lg::memory_create<lg::LstmMemory>(num_in, hidden, w_ih, w_hh, b_ih, b_hh, device_id, out);
}

int lg_lstm_load_device(lg_lstm *l, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, void *stream) {
    return lg::memory_load_device<lg::LstmMemory>(l, w_ih, w_hh, b_ih, b_hh, stream);
}

int lg_lstm_destroy(lg_lstm *l) { return lg::memory_destroy<lg::LstmMemory>(l); }

int lg_lstm_step(const lg_lstm *l_a, const lg_lstm *l_c, const float *x_a, const float *x_c, const uint8_t *reset,
                 const float *h_in_a, const float *c_in_a, float *h_out_a, float *c_out_a,
                 const float *h_in_c, const float *c_in_c, float *h_out_c, float *c_out_c, int32_t num_envs, void *stream) {
    const int rc = lg::lstm_step_check<lg::LstmMemory>(l_a, l_c, x_a, x_c, h_in_a, c_in_a, h_out_a, c_out_a, h_in_c, c_in_c, h_out_c, c_out_c, num_envs);
    if (rc) return rc;
    lg::LstmArgs A = {};
    if (l_a) lg::fill_lstm_role(A.role[0], l_a, x_a, h_in_a, c_in_a, h_out_a, c_out_a);
    if (l_c) lg::fill_lstm_role(A.role[1], l_c, x_c, h_in_c, c_in_c, h_out_c, c_out_c);
    A.reset = reset;
    A.num_envs = num_envs;
    A.blocks = (num_envs + LG_LSTM_BLOCK_ENVS - 1) / LG_LSTM_BLOCK_ENVS;
    A.first_role = l_a ? 0 : 1;
    const int roles = (l_a ? 1 : 0) + (l_c ? 1 : 0);
    const int hidden = max(l_a ? l_a->hidden : 0, l_c ? l_c->hidden : 0), ksteps = max(l_a ? l_a->ksteps : 0, l_c ? l_c->ksteps : 0);
    hipLaunchKernelGGL(lg::k_lstm_cell, dim3(roles * A.blocks), dim3(2 * hidden), lg::cell_lds_bytes(ksteps), (hipStream_t)stream, A);
    HIP_TRY(hipGetLastError());
    return 0;
}

int lg_lstm_actor_create(const int32_t dims[5], int32_t device_id, lg_lstm_actor **out) { return lg::actor_create<lg::LstmActor>(dims, device_id, out); }

int lg_lstm_actor_load_device(lg_lstm_actor *a, const float *const weights[4], const float *const biases[4], const float *std, void *stream) {
    return lg::actor_load_device<lg::LstmActor>(a, weights, biases, std, stream);
}

int lg_lstm_actor_destroy(lg_lstm_actor *a) { return lg::actor_destroy<lg::LstmActor>(a); }

int lg_lstm_actor_act(const lg_lstm_actor *a, const float *h, float *actions, float *mean, int32_t num_envs, uint64_t seed, int64_t step,
                      const int64_t *step_counter, int32_t deterministic, void *stream) {
    return lg::actor_act<lg::LstmActor>(a, h, actions, mean, num_envs, seed, step, step_counter, deterministic, stream);
}

}  // extern "C"
