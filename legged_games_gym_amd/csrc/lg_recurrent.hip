// lg_recurrent.hip -- k_lstm_cell / k_lstm_pack and their entry points (include/legged_recurrent.h): the two LSTM memories of a recurrent
// policy advanced by one rollout step in one launch.  Operand layout and lane maps: lg_recurrent.h.  A translation unit of its own: the
// code hipcc generates for the other units' kernels does not depend on it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lg_device.h"             // rand4: the Philox stream of the actor kernels
#include "lg_recurrent.h"
#include "lg_lstm_actor_body.h"      // the actor MLP of k_lstm_actor, shared with the game layer's recurrent actor launch
#include "lg_lstm_cell_body.h"       // the cell of k_lstm_cell, shared with the cell launch of the decentralised game
#include "../../include/legged_recurrent.h"

#define HIP_TRY(x) do { hipError_t _e = (x); if (_e != hipSuccess) return lg::fail(-10, "HIP error: %s", hipGetErrorString(_e)); } while (0)

namespace lg {


// [w_ih | w_hh] (torch.nn.LSTM layout, gate order i, f, g, o) -> wp, b_ih + b_hh -> bp.  One thread per float4 of the packed layout.
__global__ void __launch_bounds__(256) k_lstm_pack(const float *__restrict__ w_ih, const float *__restrict__ w_hh, const float *__restrict__ b_ih,
                                                   const float *__restrict__ b_hh, float4 *__restrict__ wp, float4 *__restrict__ bp,
                                                   const int num_in, const int hidden, const int ksteps) {
    const int n_w = (hidden / 32) * ksteps * 64;
    const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx < n_w) {
        const int lane = idx & 63, s = (idx >> 6) % ksteps, w = (idx >> 6) / ksteps;
        const int unit = 32 * w + (lane & 31), k = 2 * s + (lane >> 5);
        float v[4];
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int row = g * hidden + unit;
            v[g] = k < num_in ? w_ih[(size_t)row * num_in + k] : (k < num_in + hidden ? w_hh[(size_t)row * hidden + (k - num_in)] : 0.0f);
        }
        wp[idx] = make_float4(v[0], v[1], v[2], v[3]);
    } else if (idx < n_w + hidden) {
        const int unit = idx - n_w;
        bp[unit] = make_float4(b_ih[unit] + b_hh[unit], b_ih[hidden + unit] + b_hh[hidden + unit],
                               b_ih[2 * hidden + unit] + b_hh[2 * hidden + unit], b_ih[3 * hidden + unit] + b_hh[3 * hidden + unit]);
    }
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
    const int n_w = out_pad * in;
    const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (idx < n_w) {
        const int lane = idx & 63, ks = in / 2, s = (idx >> 6) % ks, o = (idx >> 6) / ks;
        const int unit = 32 * o + (lane & 31), k = 2 * s + (lane >> 5);
        wp[idx] = unit < out ? w[(size_t)unit * in + k] : 0.0f;
    } else if (idx < n_w + out_pad) {
        const int unit = idx - n_w;
        bp[unit] = unit < out ? b[unit] : 0.0f;
    }
}

__global__ void __launch_bounds__(64 * LG_LSTM_ACTOR_WAVES) k_lstm_actor(const LstmActorArgs A) {
    extern __shared__ float lds[];                    // two activation buffers [max_width][LG_LSTM_LD], then the noise [32][16]
    float *xa = lds, *xb = lds + (size_t)A.max_width * LG_LSTM_LD, *ns = xb + (size_t)A.max_width * LG_LSTM_LD;
    lstm_actor_body<LG_LSTM_ACTOR_WAVES, 4>(A, (int)blockIdx.x, xa, xb, ns, LstmActorStores{});      // lg_lstm_actor_body.h
}

static size_t actor_lds_bytes(const int max_width) { return ((size_t)2 * max_width * LG_LSTM_LD + 32 * 16) * sizeof(float); }
static size_t lds_bytes(const int ksteps) { return (size_t)2 * ksteps * LG_LSTM_LD * sizeof(float); }
static const int LSTM_MAX_KSTEPS = (LG_LSTM_MAX_IN + LG_LSTM_MAX_HIDDEN) / 2;

static int pack(lg_lstm *l, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, hipStream_t stream) {
    const int total = (l->hidden / 32) * l->ksteps * 64 + l->hidden;
    hipLaunchKernelGGL(k_lstm_pack, dim3((total + 255) / 256), dim3(256), 0, stream, w_ih, w_hh, b_ih, b_hh, (float4 *)l->d_wp, (float4 *)l->d_bp,
                       l->num_in, l->hidden, l->ksteps);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace lg

extern "C" {

int lg_lstm_create(int32_t num_in, int32_t hidden, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                   int32_t device_id, lg_lstm **out) {
    if (!out || !w_ih || !w_hh || !b_ih || !b_hh) return lg::fail(-1, "lg_lstm_create: null argument%s", "");
    *out = nullptr;
    if (num_in < 1 || num_in > LG_LSTM_MAX_IN)
        return lg::fail(-4, "lg_lstm_create: num_in must be 1 .. 256%s", "");
    if (hidden < 32 || hidden > LG_LSTM_MAX_HIDDEN || hidden % 32)
        return lg::fail(-4, "lg_lstm_create: hidden must be a multiple of 32 in 32 .. 256 (one layer, LSTM only)%s", "");
    HIP_TRY(hipSetDevice(device_id));
    // the staged [x | h] block of the largest shape is above the 64 KB a kernel gets without asking
    HIP_TRY(hipFuncSetAttribute((const void *)lg::k_lstm_cell, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lg::lds_bytes(lg::LSTM_MAX_KSTEPS)));
    lg_lstm *l = new lg_lstm();
    l->num_in = num_in; l->hidden = hidden; l->ksteps = (num_in + hidden + 1) / 2; l->device = device_id;
    l->d_wp = l->d_bp = nullptr;
    const size_t n_ih = (size_t)4 * hidden * num_in, n_hh = (size_t)4 * hidden * hidden, n_b = (size_t)4 * hidden;
    float *raw = nullptr;
    int rc = 0;
    auto body = [&]() -> int {
        HIP_TRY(hipMalloc(&l->d_wp, (size_t)(hidden / 32) * l->ksteps * 64 * 4 * sizeof(float)));
        HIP_TRY(hipMalloc(&l->d_bp, n_b * sizeof(float)));
        HIP_TRY(hipMalloc(&raw, (n_ih + n_hh + 2 * n_b) * sizeof(float)));
        HIP_TRY(hipMemcpy(raw, w_ih, n_ih * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(raw + n_ih, w_hh, n_hh * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(raw + n_ih + n_hh, b_ih, n_b * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(raw + n_ih + n_hh + n_b, b_hh, n_b * sizeof(float), hipMemcpyHostToDevice));
        const int prc = lg::pack(l, raw, raw + n_ih, raw + n_ih + n_hh, raw + n_ih + n_hh + n_b, nullptr);
        if (prc) return prc;
        HIP_TRY(hipStreamSynchronize(nullptr));
        return 0;
    };
    rc = body();
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

int lg_lstm_load_device(lg_lstm *l, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, void *stream) {
    if (!l || !w_ih || !w_hh || !b_ih || !b_hh) return lg::fail(-1, "lg_lstm_load_device: null argument%s", "");
    return lg::pack(l, w_ih, w_hh, b_ih, b_hh, (hipStream_t)stream);
}

int lg_lstm_destroy(lg_lstm *l) {
    if (!l) return lg::fail(-1, "lg_lstm_destroy: null handle%s", "");
    (void)hipFree(l->d_wp);
    (void)hipFree(l->d_bp);
    delete l;
    return 0;
}

int lg_lstm_step(const lg_lstm *l_a, const lg_lstm *l_c, const float *x_a, const float *x_c, const uint8_t *reset,
                 const float *h_in_a, const float *c_in_a, float *h_out_a, float *c_out_a,
                 const float *h_in_c, const float *c_in_c, float *h_out_c, float *c_out_c, int32_t num_envs, void *stream) {
    if (!l_a && !l_c) return lg::fail(-1, "lg_lstm_step: both handles are null%s", "");
    if (l_a && (!x_a || !h_in_a || !c_in_a || !h_out_a || !c_out_a)) return lg::fail(-1, "lg_lstm_step: null buffer of the actor memory%s", "");
    if (l_c && (!x_c || !h_in_c || !c_in_c || !h_out_c || !c_out_c)) return lg::fail(-1, "lg_lstm_step: null buffer of the critic memory%s", "");
    if (num_envs < 1) return lg::fail(-2, "lg_lstm_step: num_envs must be >= 1%s", "");
    auto aliased = [](const float *h_in, const float *c_in, const float *h_out, const float *c_out) {
        return h_out == h_in || h_out == c_in || c_out == h_in || c_out == c_in || h_out == c_out;
    };
    if ((l_a && aliased(h_in_a, c_in_a, h_out_a, c_out_a)) || (l_c && aliased(h_in_c, c_in_c, h_out_c, c_out_c)))
        return lg::fail(-2, "lg_lstm_step: h_out / c_out must not alias h_in / c_in (other workgroups read them as the K operand)%s", "");
    if (l_a && l_c && l_a->device != l_c->device) return lg::fail(-2, "lg_lstm_step: the two memories live on different devices%s", "");
    lg::LstmArgs A = {};
    auto fill = [](lg::LstmRole &R, const lg_lstm *l, const float *x, const float *h_in, const float *c_in, float *h_out, float *c_out) {
        R.x = x; R.h_in = h_in; R.c_in = c_in; R.h_out = h_out; R.c_out = c_out;
        R.wp = l->d_wp; R.bp = l->d_bp; R.num_in = l->num_in; R.hidden = l->hidden; R.ksteps = l->ksteps;
    };
    if (l_a) fill(A.role[0], l_a, x_a, h_in_a, c_in_a, h_out_a, c_out_a);
    if (l_c) fill(A.role[1], l_c, x_c, h_in_c, c_in_c, h_out_c, c_out_c);
    A.reset = reset;
    A.num_envs = num_envs;
    A.blocks = (num_envs + LG_LSTM_BLOCK_ENVS - 1) / LG_LSTM_BLOCK_ENVS;
    A.first_role = l_a ? 0 : 1;
    const int roles = (l_a ? 1 : 0) + (l_c ? 1 : 0);
    const int hidden = max(l_a ? l_a->hidden : 0, l_c ? l_c->hidden : 0), ksteps = max(l_a ? l_a->ksteps : 0, l_c ? l_c->ksteps : 0);
    hipLaunchKernelGGL(lg::k_lstm_cell, dim3(roles * A.blocks), dim3(2 * hidden), lg::lds_bytes(ksteps), (hipStream_t)stream, A);
    HIP_TRY(hipGetLastError());
    return 0;
}

int lg_lstm_actor_create(const int32_t dims[5], int32_t device_id, lg_lstm_actor **out) {
    if (!dims || !out) return lg::fail(-1, "lg_lstm_actor_create: null argument%s", "");
    *out = nullptr;
    if (dims[0] < 32 || dims[0] > LG_LSTM_MAX_HIDDEN || dims[0] % 32)
        return lg::fail(-4, "lg_lstm_actor_create: the input width must be a memory's hidden size (a multiple of 32 in 32 .. 256)%s", "");
    for (int i = 1; i <= 3; i++)
        if (dims[i] < 32 || dims[i] > 512 || dims[i] % 32) return lg::fail(-4, "lg_lstm_actor_create: hidden widths must be multiples of 32 in 32 .. 512%s", "");
    if (dims[4] < 1 || dims[4] > 16) return lg::fail(-4, "lg_lstm_actor_create: 1 .. 16 actions%s", "");
    HIP_TRY(hipSetDevice(device_id));
    lg_lstm_actor *a = new lg_lstm_actor();
    size_t at = 0;
    a->max_width = 0;
    for (int i = 0; i < 5; i++) {
        a->dims[i] = dims[i]; a->pad[i] = (dims[i] + 31) / 32 * 32;
        if (i < 4 && a->pad[i] > a->max_width) a->max_width = a->pad[i];
    }
    for (int i = 0; i < 4; i++) {
        a->w_off[i] = at; at += (size_t)a->pad[i + 1] * dims[i];
        a->b_off[i] = at; at += (size_t)a->pad[i + 1];
    }
    a->device = device_id; a->d_p = a->d_std = nullptr;
    if (hipFuncSetAttribute((const void *)lg::k_lstm_actor, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lg::actor_lds_bytes(512)) != hipSuccess ||
        hipMalloc(&a->d_p, at * sizeof(float)) != hipSuccess || hipMalloc(&a->d_std, 16 * sizeof(float)) != hipSuccess ||
        hipMemset(a->d_p, 0, at * sizeof(float)) != hipSuccess || hipMemset(a->d_std, 0, 16 * sizeof(float)) != hipSuccess) {
        if (a->d_p) (void)hipFree(a->d_p);
        if (a->d_std) (void)hipFree(a->d_std);
        delete a;
        return lg::fail(-10, "lg_lstm_actor_create: device allocation failed%s", "");
    }
    *out = a;
    return 0;
}

int lg_lstm_actor_load_device(lg_lstm_actor *a, const float *const weights[4], const float *const biases[4], const float *std, void *stream) {
    if (!a || !weights || !biases || !std) return lg::fail(-1, "lg_lstm_actor_load_device: null argument%s", "");
    for (int i = 0; i < 4; i++) if (!weights[i] || !biases[i]) return lg::fail(-1, "lg_lstm_actor_load_device: null layer%s", "");
    for (int i = 0; i < 4; i++) {
        const int total = a->pad[i + 1] * a->dims[i] + a->pad[i + 1];
        hipLaunchKernelGGL(lg::k_lstm_actor_pack, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, weights[i], biases[i],
                           a->d_p + a->w_off[i], a->d_p + a->b_off[i], a->dims[i], a->dims[i + 1], a->pad[i + 1]);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(a->d_std, std, a->dims[4] * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

int lg_lstm_actor_destroy(lg_lstm_actor *a) {
    if (!a) return lg::fail(-1, "lg_lstm_actor_destroy: null handle%s", "");
    (void)hipFree(a->d_p);
    (void)hipFree(a->d_std);
    delete a;
    return 0;
}

int lg_lstm_actor_act(const lg_lstm_actor *a, const float *h, float *actions, float *mean, int32_t num_envs, uint64_t seed, int64_t step,
                      const int64_t *step_counter, int32_t deterministic, void *stream) {
    if (!a || !h || !actions) return lg::fail(-1, "lg_lstm_actor_act: null argument%s", "");
    if (num_envs < 1) return lg::fail(-2, "lg_lstm_actor_act: num_envs must be >= 1%s", "");
    lg::LstmActorArgs A = {};
    A.h = h; A.p = a->d_p; A.std = a->d_std; A.actions = actions; A.mean = mean; A.step_counter = step_counter;
    A.seed = seed; A.step = step; A.num_envs = num_envs; A.deterministic = deterministic; A.max_width = a->max_width;
    for (int i = 0; i < 5; i++) { A.dims[i] = a->dims[i]; A.pad[i] = a->pad[i]; }
    for (int i = 0; i < 4; i++) { A.w_off[i] = (uint32_t)a->w_off[i]; A.b_off[i] = (uint32_t)a->b_off[i]; }
    hipLaunchKernelGGL(lg::k_lstm_actor, dim3((num_envs + 31) / 32), dim3(64 * LG_LSTM_ACTOR_WAVES), lg::actor_lds_bytes(a->max_width), (hipStream_t)stream, A);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
