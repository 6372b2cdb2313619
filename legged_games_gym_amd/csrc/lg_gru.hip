// lg_gru.hip -- k_gru_cell / k_gru_pack and their entry points (include/legged_recurrent_gru.h): the two GRU memories of a recurrent policy
// advanced by one rollout step in one launch.  The only translation unit of liblegged_gru.so: it links against nothing of the main library
// and owns its handles.  The actor MLP behind a GRU memory reads only h, so the main library's lg_lstm_actor_act serves unchanged.
//
// The launch, the staged [x | h_in] block, the lane maps and the k-loop are k_lstm_cell's (lg_recurrent.h); the pack kernel and the
// epilogue are the GRU's (lg_gru_cell_body.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lg_device.h"             // f32x16
#include "lg_recurrent.h"          // LG_LSTM_LD: the staged block and the lane maps
#include "lg_lstm_cell_body.h"     // stage_xh, lstm_sigmoid, lstm_tanh
#include "lg_gru_cell_body.h"
#include "lg_gru.h"                // struct lg_gru
#include "lg_lib_error.h"          // g_error, refuse, HIP_TRY
#include "lg_memory_host.h"        // create / load_device / destroy of the handle, written once for the three cell libraries
#include "../../include/legged_recurrent_gru.h"

namespace lg {

struct GruArgs {
    GruRole role[2];               // actor memory, critic memory
    const uint8_t *reset;
    int32_t num_envs, blocks;      // workgroups per present role
    int32_t first_role, _pad;      // role of workgroups 0 .. blocks - 1 (the other, when present, follows)
};

// torch.nn.GRU layout (gate rows r, z, n) -> wp[hidden / 32][ksteps][64] float4 (r, z, n_x, n_h): element (w, s, l) is unit 32 w + (l & 31)
// at k = 2 s + (l >> 5); k < num_in reads w_ih and leaves n_h zero, num_in <= k < K reads w_hh and leaves n_x zero, the pad k = K of an odd K
// is zeros.  bp[hidden] float4 (b_ir + b_hr, b_iz + b_hz, b_in, b_hn).  One thread per float4.
__global__ void __launch_bounds__(256) k_gru_pack(const float *__restrict__ w_ih, const float *__restrict__ w_hh, const float *__restrict__ b_ih,
                                                  const float *__restrict__ b_hh, float4 *__restrict__ wp, float4 *__restrict__ bp,
                                                  const int num_in, const int hidden, const int ksteps) {
    const int n_w = (hidden / 32) * ksteps * 64;
    const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx < n_w) {
        const int lane = idx & 63, s = (idx >> 6) % ksteps, w = (idx >> 6) / ksteps;
        const int unit = 32 * w + (lane & 31), k = 2 * s + (lane >> 5);
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (k < num_in) {
            v.x = w_ih[(size_t)unit * num_in + k];
            v.y = w_ih[(size_t)(hidden + unit) * num_in + k];
            v.z = w_ih[(size_t)(2 * hidden + unit) * num_in + k];
        } else if (k < num_in + hidden) {
            v.x = w_hh[(size_t)unit * hidden + (k - num_in)];
            v.y = w_hh[(size_t)(hidden + unit) * hidden + (k - num_in)];
            v.w = w_hh[(size_t)(2 * hidden + unit) * hidden + (k - num_in)];
        }
        wp[idx] = v;
    } else if (idx < n_w + hidden) {
        const int unit = idx - n_w;
        bp[unit] = make_float4(b_ih[unit] + b_hh[unit], b_ih[hidden + unit] + b_hh[hidden + unit], b_ih[2 * hidden + unit], b_hh[2 * hidden + unit]);
    }
}

__global__ void __launch_bounds__(2 * LG_GRU_MAX_HIDDEN) k_gru_cell(const GruArgs A) {
    extern __shared__ float xs[];                                                 // [2 ksteps][LG_LSTM_LD]
    const int second = (int)blockIdx.x >= A.blocks;
    const int blk = (int)blockIdx.x - (second ? A.blocks : 0);
    if ((second ? 1 : A.first_role) == 0) gru_cell_role(A.role[0], A.reset, A.num_envs, blk, xs);
    else gru_cell_role(A.role[1], A.reset, A.num_envs, blk, xs);
}

struct GruMemory {                 // lg_memory_host.h: the traits of lg_gru
    using Handle = lg_gru;
    static constexpr int GATES = 3, MAX_IN = LG_GRU_MAX_IN, MAX_HIDDEN = LG_GRU_MAX_HIDDEN;
    static const char *name() { return "lg_gru"; }
    static const char *hidden_note() { return " (one layer)"; }
    static const void *cell_kernel() { return (const void *)k_gru_cell; }               // 67 584 B of staged [x | h] at the largest shape
    template <class... Args> static void pack(const dim3 grid, hipStream_t stream, Args... args) { hipLaunchKernelGGL(k_gru_pack, grid, dim3(256), 0, stream, args...); }
    static int error(const int code, const char *msg) { return refuse(code, "%s", msg); }
};

}  // namespace lg

extern "C" {

int lg_gru_create(int32_t num_in, int32_t hidden, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                  int32_t device_id, lg_gru **out) {
    return lg::memory_create<lg::GruMemory>(num_in, hidden, w_ih, w_hh, b_ih, b_hh, device_id, out);
}

int lg_gru_load_device(lg_gru *l, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, void *stream) {
    return lg::memory_load_device<lg::GruMemory>(l, w_ih, w_hh, b_ih, b_hh, stream);
}

int lg_gru_destroy(lg_gru *l) { return lg::memory_destroy<lg::GruMemory>(l); }

int lg_gru_step(const lg_gru *l_a, const lg_gru *l_c, const float *x_a, const float *x_c, const uint8_t *reset,
                const float *h_in_a, float *h_out_a, const float *h_in_c, float *h_out_c, int32_t num_envs, void *stream) {
    if (!l_a && !l_c) return lg::refuse(-1, "lg_gru_step: both handles are null");
    if (l_a && (!x_a || !h_in_a || !h_out_a)) return lg::refuse(-1, "lg_gru_step: null buffer of the actor memory");
    if (l_c && (!x_c || !h_in_c || !h_out_c)) return lg::refuse(-1, "lg_gru_step: null buffer of the critic memory");
    if (num_envs < 1) return lg::refuse(-2, "lg_gru_step: num_envs must be >= 1");
    if ((l_a && h_out_a == h_in_a) || (l_c && h_out_c == h_in_c))
        return lg::refuse(-2, "lg_gru_step: h_out must not alias h_in (the epilogue reads h_in while other waves write h_out)");
    if (l_a && l_c && l_a->device != l_c->device) return lg::refuse(-2, "lg_gru_step: the two memories live on different devices");
    lg::GruArgs A = {};
    auto fill = [](lg::GruRole &R, const lg_gru *l, const float *x, const float *h_in, float *h_out) {
        R.x = x; R.h_in = h_in; R.h_out = h_out;
        R.wp = l->d_wp; R.bp = l->d_bp; R.num_in = l->num_in; R.hidden = l->hidden; R.ksteps = l->ksteps;
    };
    if (l_a) fill(A.role[0], l_a, x_a, h_in_a, h_out_a);
    if (l_c) fill(A.role[1], l_c, x_c, h_in_c, h_out_c);
    A.reset = reset;
    A.num_envs = num_envs;
    A.blocks = (num_envs + LG_GRU_BLOCK_ENVS - 1) / LG_GRU_BLOCK_ENVS;
    A.first_role = l_a ? 0 : 1;
    const int roles = (l_a ? 1 : 0) + (l_c ? 1 : 0);
    const int hidden = max(l_a ? l_a->hidden : 0, l_c ? l_c->hidden : 0), ksteps = max(l_a ? l_a->ksteps : 0, l_c ? l_c->ksteps : 0);
    hipLaunchKernelGGL(lg::k_gru_cell, dim3(roles * A.blocks), dim3(2 * hidden), lg::cell_lds_bytes(ksteps), (hipStream_t)stream, A);
    HIP_TRY(hipGetLastError());
    return 0;
}

const char *lg_gru_last_error(void) { return lg::g_error; }

}  // extern "C"
