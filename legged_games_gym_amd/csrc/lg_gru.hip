// lg_gru.hip -- k_gru_cell / k_gru_pack and their entry points (include/legged_recurrent_gru.h): the two GRU memories of a recurrent policy
// advanced by one rollout step in one launch.  The only translation unit of liblegged_gru.so: it links against nothing of the main library
// and owns its handles.  The actor MLP behind a GRU memory reads only h, so the main library's lg_lstm_actor_act serves unchanged.
//
// The launch, the staged [x | h_in] block, the lane maps and the k-loop are k_lstm_cell's (lg_recurrent.h); the pack kernel and the
// epilogue are the GRU's (lg_gru_cell_body.h).
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "lg_device.h"             // f32x16
#include "lg_recurrent.h"          // LG_LSTM_LD: the staged block and the lane maps
#include "lg_lstm_cell_body.h"     // lstm_sigmoid, lstm_tanh
#include "lg_gru_cell_body.h"
#include "lg_gru.h"                // struct lg_gru
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

static size_t gru_lds_bytes(const int ksteps) { return (size_t)2 * ksteps * LG_LSTM_LD * sizeof(float); }
static const int GRU_MAX_KSTEPS = (LG_GRU_MAX_IN + LG_GRU_MAX_HIDDEN) / 2;

static thread_local char g_error[512] = "";
static int refuse(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}

}  // namespace lg

#define HIP_TRY(x) do { hipError_t _e = (x); if (_e != hipSuccess) return lg::refuse(-10, "HIP error: %s", hipGetErrorString(_e)); } while (0)

namespace lg {

static int gru_pack(lg_gru *l, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, hipStream_t stream) {
    const int total = (l->hidden / 32) * l->ksteps * 64 + l->hidden;
    hipLaunchKernelGGL(k_gru_pack, dim3((total + 255) / 256), dim3(256), 0, stream, w_ih, w_hh, b_ih, b_hh, (float4 *)l->d_wp, (float4 *)l->d_bp,
                       l->num_in, l->hidden, l->ksteps);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace lg

extern "C" {

int lg_gru_create(int32_t num_in, int32_t hidden, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                  int32_t device_id, lg_gru **out) {
    if (!out || !w_ih || !w_hh || !b_ih || !b_hh) return lg::refuse(-1, "lg_gru_create: null argument");
    *out = nullptr;
    if (num_in < 1 || num_in > LG_GRU_MAX_IN)
        return lg::refuse(-4, "lg_gru_create: num_in must be 1 .. 256");
    if (hidden < 32 || hidden > LG_GRU_MAX_HIDDEN || hidden % 32)
        return lg::refuse(-4, "lg_gru_create: hidden must be a multiple of 32 in 32 .. 256 (one layer)");
    HIP_TRY(hipSetDevice(device_id));
    // the staged [x | h] block of the largest shape (67 584 B) is above the 64 KB a kernel gets without asking
    HIP_TRY(hipFuncSetAttribute((const void *)lg::k_gru_cell, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lg::gru_lds_bytes(lg::GRU_MAX_KSTEPS)));
    lg_gru *l = new lg_gru();
    l->num_in = num_in; l->hidden = hidden; l->ksteps = (num_in + hidden + 1) / 2; l->device = device_id;
    l->d_wp = l->d_bp = nullptr;
    const size_t n_ih = (size_t)3 * hidden * num_in, n_hh = (size_t)3 * hidden * hidden, n_b = (size_t)3 * hidden;
    float *raw = nullptr;
    auto body = [&]() -> int {
        HIP_TRY(hipMalloc(&l->d_wp, (size_t)(hidden / 32) * l->ksteps * 64 * 4 * sizeof(float)));
        HIP_TRY(hipMalloc(&l->d_bp, (size_t)4 * hidden * sizeof(float)));
        HIP_TRY(hipMalloc(&raw, (n_ih + n_hh + 2 * n_b) * sizeof(float)));
        HIP_TRY(hipMemcpy(raw, w_ih, n_ih * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(raw + n_ih, w_hh, n_hh * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(raw + n_ih + n_hh, b_ih, n_b * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(raw + n_ih + n_hh + n_b, b_hh, n_b * sizeof(float), hipMemcpyHostToDevice));
        const int prc = lg::gru_pack(l, raw, raw + n_ih, raw + n_ih + n_hh, raw + n_ih + n_hh + n_b, nullptr);
        if (prc) return prc;
        HIP_TRY(hipStreamSynchronize(nullptr));
        return 0;
    };
    const int rc = body();
    if (raw) (void)hipFree(raw);
    if (rc) {
        if (l->d_wp) (void)hipFree(l->d_wp);
        if (l->d_bp) (void)hipFree(l->d_bp);
        delete l;
        return rc;
    }
    *out = l;
    return 0;
}

int lg_gru_load_device(lg_gru *l, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, void *stream) {
    if (!l || !w_ih || !w_hh || !b_ih || !b_hh) return lg::refuse(-1, "lg_gru_load_device: null argument");
    return lg::gru_pack(l, w_ih, w_hh, b_ih, b_hh, (hipStream_t)stream);
}

int lg_gru_destroy(lg_gru *l) {
    if (!l) return lg::refuse(-1, "lg_gru_destroy: null handle");
    (void)hipFree(l->d_wp);
    (void)hipFree(l->d_bp);
    delete l;
    return 0;
}

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
    hipLaunchKernelGGL(lg::k_gru_cell, dim3(roles * A.blocks), dim3(2 * hidden), lg::gru_lds_bytes(ksteps), (hipStream_t)stream, A);
    HIP_TRY(hipGetLastError());
    return 0;
}

const char *lg_gru_last_error(void) { return lg::g_error; }

}  // extern "C"
