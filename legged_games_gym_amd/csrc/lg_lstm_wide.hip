// lg_lstm_wide.hip -- k_lstm_wide_cell / k_lstm_wide_actor, their pack kernels and entry points (include/legged_recurrent_wide.h): the two
// LSTM memories of a recurrent policy with up to 512 units advanced by one rollout step in one launch, and the actor MLP behind such a
// memory.  The only translation unit of liblegged_lstm_wide.so: it links against nothing of the main library and owns its handles.
//
// The cell splits a memory's units over workgroups, not over more waves of one: a workgroup is 32 env rows x one unit group of up to 256
// units (8 waves).  Every workgroup stages the whole [x | h_in] block of its rows, then wave w of group g runs lg_lstm_cell_body.h's
// k-ordered chain for units 256 g + 32 w ..: the same products in the same order from the same packed operands (lg_recurrent.h), the same
// epilogue.  h_out never aliases h_in, so the groups need no exchange.  The body is restated here and not shared: lstm_cell_role takes its
// wave index, its staging stride and its surplus-wave rule from the one-workgroup launch, and the rows of kernel_resources.txt and
// kernel_resources_dec_game_recurrent.txt that it compiles into are pinned.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "lg_device.h"             // rand4, f32x16, LG_DEV
#include "lg_recurrent.h"          // LstmRole, LstmActorArgs, LG_LSTM_LD: operand layout and lane maps
#include "lg_lstm_actor_body.h"    // the actor MLP chain, unchanged
#include "lg_lstm_cell_body.h"     // lstm_sigmoid, lstm_tanh
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

// One role's workgroup: env rows 32 blk .. 32 blk + 31, units 256 grp .. of the role's memory.  All waves of the workgroup stage (the
// launch is sized for the widest group of the widest role); a wave past the group's units then only meets the barrier.
__device__ __forceinline__ void lstm_wide_role(const LstmRole &R, const uint8_t *__restrict__ reset, const int num_envs, const int blk, const int grp,
                                               float *xs) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = (int)blockDim.x;
    const int I = R.num_in, H = R.hidden, K = I + H;
    const int env0 = 32 * blk;
    // stage [x | h_in] of the 32 rows as xs[k][row]; rows past num_envs and the pad row k = K are zeros, a reset row's h is zero
    for (int e = tid; e < 32 * I; e += nthreads) {
        const int row = e / I, k = e - row * I, env = env0 + row;
        xs[k * LG_LSTM_LD + row] = env < num_envs ? R.x[(size_t)env * I + k] : 0.0f;
    }
    for (int e = tid; e < 32 * H; e += nthreads) {
        const int row = e / H, k = e - row * H, env = env0 + row;
        const bool live = env < num_envs && !(reset && reset[env]);
        xs[(I + k) * LG_LSTM_LD + row] = live ? R.h_in[(size_t)env * H + k] : 0.0f;
    }
    if ((K & 1) && tid < 32) xs[K * LG_LSTM_LD + tid] = 0.0f;                         // the pad row of an odd K
    __syncthreads();
    const int gw = LG_LSTM_WIDE_GROUP_WAVES * grp + wave;                             // the wave's 32 units among the memory's
    if (wave >= LG_LSTM_WIDE_GROUP_WAVES || gw >= H / 32) return;

    const int unit = 32 * gw + (lane & 31);
    const float4 b = ((const float4 *)R.bp)[unit];
    f32x16 acc_i, acc_f, acc_g, acc_o;
#pragma unroll
    for (int r = 0; r < 16; r++) { acc_i[r] = b.x; acc_f[r] = b.y; acc_g[r] = b.z; acc_o[r] = b.w; }
    const float4 *__restrict__ wp = (const float4 *)R.wp + (size_t)gw * R.ksteps * 64 + lane;
    const float *xl = xs + (lane >> 5) * LG_LSTM_LD + (lane & 31);
#define LG_LSTM_KSTEP(W_, A_) \
    acc_i = __builtin_amdgcn_mfma_f32_32x32x2f32(A_, W_.x, acc_i, 0, 0, 0); acc_f = __builtin_amdgcn_mfma_f32_32x32x2f32(A_, W_.y, acc_f, 0, 0, 0); \
    acc_g = __builtin_amdgcn_mfma_f32_32x32x2f32(A_, W_.z, acc_g, 0, 0, 0); acc_o = __builtin_amdgcn_mfma_f32_32x32x2f32(A_, W_.w, acc_o, 0, 0, 0);
    int s = 0;
    for (; s + 4 <= R.ksteps; s += 4) {           // four k-steps' operands in flight
        const float4 w0 = wp[(size_t)s * 64], w1 = wp[(size_t)(s + 1) * 64], w2 = wp[(size_t)(s + 2) * 64], w3 = wp[(size_t)(s + 3) * 64];
        const float a0 = xl[2 * s * LG_LSTM_LD], a1 = xl[(2 * s + 2) * LG_LSTM_LD], a2 = xl[(2 * s + 4) * LG_LSTM_LD], a3 = xl[(2 * s + 6) * LG_LSTM_LD];
        LG_LSTM_KSTEP(w0, a0) LG_LSTM_KSTEP(w1, a1) LG_LSTM_KSTEP(w2, a2) LG_LSTM_KSTEP(w3, a3)
    }
    for (; s < R.ksteps; s++) {
        const float4 w = wp[(size_t)s * 64];
        const float a = xl[2 * s * LG_LSTM_LD];
        LG_LSTM_KSTEP(w, a)
    }
#undef LG_LSTM_KSTEP
    // cell update straight from the accumulators: register r is env row (r & 3) + 8 (r >> 2) + 4 (lane >> 5), column = unit
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int env = env0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (env < num_envs) {
            const size_t o = (size_t)env * H + unit;
            const float c_prev = (reset && reset[env]) ? 0.0f : R.c_in[o];
            const float c = lstm_sigmoid(acc_f[r]) * c_prev + lstm_sigmoid(acc_i[r]) * lstm_tanh(acc_g[r]);
            R.c_out[o] = c;
            R.h_out[o] = lstm_sigmoid(acc_o[r]) * lstm_tanh(c);
        }
    }
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

__global__ void __launch_bounds__(64 * LG_LSTM_WIDE_ACTOR_WAVES) k_lstm_wide_actor(const LstmActorArgs A) {
    extern __shared__ float lds[];                    // two activation buffers [max_width][LG_LSTM_LD], then the noise [32][16]
    float *xa = lds, *xb = lds + (size_t)A.max_width * LG_LSTM_LD, *ns = xb + (size_t)A.max_width * LG_LSTM_LD;
    lstm_actor_body<LG_LSTM_WIDE_ACTOR_WAVES, 16>(A, (int)blockIdx.x, xa, xb, ns, LstmActorStores{});     // lg_lstm_actor_body.h
}

static size_t wide_actor_lds_bytes(const int max_width) { return ((size_t)2 * max_width * LG_LSTM_LD + 32 * 16) * sizeof(float); }
static size_t wide_lds_bytes(const int ksteps) { return (size_t)2 * ksteps * LG_LSTM_LD * sizeof(float); }
static const int LSTM_WIDE_MAX_KSTEPS = (LG_LSTM_WIDE_MAX_IN + LG_LSTM_WIDE_MAX_HIDDEN) / 2;

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

static int wide_pack(lg_lstm_wide *l, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, hipStream_t stream) {
    const int total = (l->hidden / 32) * l->ksteps * 64 + l->hidden;
    hipLaunchKernelGGL(k_lstm_wide_pack, dim3((total + 255) / 256), dim3(256), 0, stream, w_ih, w_hh, b_ih, b_hh, (float4 *)l->d_wp, (float4 *)l->d_bp,
                       l->num_in, l->hidden, l->ksteps);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace lg

extern "C" {

int lg_lstm_wide_create(int32_t num_in, int32_t hidden, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                        int32_t device_id, lg_lstm_wide **out) {
    if (!out || !w_ih || !w_hh || !b_ih || !b_hh) return lg::refuse(-1, "lg_lstm_wide_create: null argument");
    *out = nullptr;
    if (num_in < 1 || num_in > LG_LSTM_WIDE_MAX_IN)
        return lg::refuse(-4, "lg_lstm_wide_create: num_in must be 1 .. 256");
    if (hidden < 32 || hidden > LG_LSTM_WIDE_MAX_HIDDEN || hidden % 32)
        return lg::refuse(-4, "lg_lstm_wide_create: hidden must be a multiple of 32 in 32 .. 512 (one layer, LSTM only)");
    HIP_TRY(hipSetDevice(device_id));
    // the staged [x | h] block of the largest shape (101 376 B) is above the 64 KB a kernel gets without asking
    HIP_TRY(hipFuncSetAttribute((const void *)lg::k_lstm_wide_cell, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lg::wide_lds_bytes(lg::LSTM_WIDE_MAX_KSTEPS)));
    lg_lstm_wide *l = new lg_lstm_wide();
    l->num_in = num_in; l->hidden = hidden; l->ksteps = (num_in + hidden + 1) / 2; l->device = device_id;
    l->d_wp = l->d_bp = nullptr;
    const size_t n_ih = (size_t)4 * hidden * num_in, n_hh = (size_t)4 * hidden * hidden, n_b = (size_t)4 * hidden;
    float *raw = nullptr;
    auto body = [&]() -> int {
        HIP_TRY(hipMalloc(&l->d_wp, (size_t)(hidden / 32) * l->ksteps * 64 * 4 * sizeof(float)));
        HIP_TRY(hipMalloc(&l->d_bp, n_b * sizeof(float)));
        HIP_TRY(hipMalloc(&raw, (n_ih + n_hh + 2 * n_b) * sizeof(float)));
        HIP_TRY(hipMemcpy(raw, w_ih, n_ih * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(raw + n_ih, w_hh, n_hh * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(raw + n_ih + n_hh, b_ih, n_b * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(raw + n_ih + n_hh + n_b, b_hh, n_b * sizeof(float), hipMemcpyHostToDevice));
        const int prc = lg::wide_pack(l, raw, raw + n_ih, raw + n_ih + n_hh, raw + n_ih + n_hh + n_b, nullptr);
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

int lg_lstm_wide_load_device(lg_lstm_wide *l, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, void *stream) {
    if (!l || !w_ih || !w_hh || !b_ih || !b_hh) return lg::refuse(-1, "lg_lstm_wide_load_device: null argument");
    return lg::wide_pack(l, w_ih, w_hh, b_ih, b_hh, (hipStream_t)stream);
}

int lg_lstm_wide_destroy(lg_lstm_wide *l) {
    if (!l) return lg::refuse(-1, "lg_lstm_wide_destroy: null handle");
    (void)hipFree(l->d_wp);
    (void)hipFree(l->d_bp);
    delete l;
    return 0;
}

int lg_lstm_wide_step(const lg_lstm_wide *l_a, const lg_lstm_wide *l_c, const float *x_a, const float *x_c, const uint8_t *reset,
                      const float *h_in_a, const float *c_in_a, float *h_out_a, float *c_out_a,
                      const float *h_in_c, const float *c_in_c, float *h_out_c, float *c_out_c, int32_t num_envs, void *stream) {
    if (!l_a && !l_c) return lg::refuse(-1, "lg_lstm_wide_step: both handles are null");
    if (l_a && (!x_a || !h_in_a || !c_in_a || !h_out_a || !c_out_a)) return lg::refuse(-1, "lg_lstm_wide_step: null buffer of the actor memory");
    if (l_c && (!x_c || !h_in_c || !c_in_c || !h_out_c || !c_out_c)) return lg::refuse(-1, "lg_lstm_wide_step: null buffer of the critic memory");
    if (num_envs < 1) return lg::refuse(-2, "lg_lstm_wide_step: num_envs must be >= 1");
    auto aliased = [](const float *h_in, const float *c_in, const float *h_out, const float *c_out) {
        return h_out == h_in || h_out == c_in || c_out == h_in || c_out == c_in || h_out == c_out;
    };
    if ((l_a && aliased(h_in_a, c_in_a, h_out_a, c_out_a)) || (l_c && aliased(h_in_c, c_in_c, h_out_c, c_out_c)))
        return lg::refuse(-2, "lg_lstm_wide_step: h_out / c_out must not alias h_in / c_in (other workgroups read them as the K operand)");
    if (l_a && l_c && l_a->device != l_c->device) return lg::refuse(-2, "lg_lstm_wide_step: the two memories live on different devices");
    lg::LstmWideArgs A = {};
    auto fill = [](lg::LstmRole &R, const lg_lstm_wide *l, const float *x, const float *h_in, const float *c_in, float *h_out, float *c_out) {
        R.x = x; R.h_in = h_in; R.c_in = c_in; R.h_out = h_out; R.c_out = c_out;
        R.wp = l->d_wp; R.bp = l->d_bp; R.num_in = l->num_in; R.hidden = l->hidden; R.ksteps = l->ksteps;
    };
    if (l_a) fill(A.role[0], l_a, x_a, h_in_a, c_in_a, h_out_a, c_out_a);
    if (l_c) fill(A.role[1], l_c, x_c, h_in_c, c_in_c, h_out_c, c_out_c);
    auto groups = [](const lg_lstm_wide *l) { return l ? (l->hidden + LG_LSTM_WIDE_GROUP_UNITS - 1) / LG_LSTM_WIDE_GROUP_UNITS : 0; };
    A.reset = reset;
    A.num_envs = num_envs;
    A.blocks = (num_envs + LG_LSTM_WIDE_BLOCK_ENVS - 1) / LG_LSTM_WIDE_BLOCK_ENVS;
    A.first_role = l_a ? 0 : 1;
    A.first_wgs = A.blocks * groups(l_a ? l_a : l_c);
    const int wgs = A.blocks * (groups(l_a) + groups(l_c));
    const int hidden = max(l_a ? l_a->hidden : 0, l_c ? l_c->hidden : 0), ksteps = max(l_a ? l_a->ksteps : 0, l_c ? l_c->ksteps : 0);
    const int waves = min(hidden / 32, LG_LSTM_WIDE_GROUP_WAVES);
    hipLaunchKernelGGL(lg::k_lstm_wide_cell, dim3(wgs), dim3(64 * waves), lg::wide_lds_bytes(ksteps), (hipStream_t)stream, A);
    HIP_TRY(hipGetLastError());
    return 0;
}

int lg_lstm_wide_actor_create(const int32_t dims[5], int32_t device_id, lg_lstm_wide_actor **out) {
    if (!dims || !out) return lg::refuse(-1, "lg_lstm_wide_actor_create: null argument");
    *out = nullptr;
    if (dims[0] < 32 || dims[0] > LG_LSTM_WIDE_MAX_HIDDEN || dims[0] % 32)
        return lg::refuse(-4, "lg_lstm_wide_actor_create: the input width must be a memory's hidden size (a multiple of 32 in 32 .. 512)");
    for (int i = 1; i <= 3; i++)
        if (dims[i] < 32 || dims[i] > 512 || dims[i] % 32) return lg::refuse(-4, "lg_lstm_wide_actor_create: hidden widths must be multiples of 32 in 32 .. 512");
    if (dims[4] < 1 || dims[4] > 16) return lg::refuse(-4, "lg_lstm_wide_actor_create: 1 .. 16 actions");
    HIP_TRY(hipSetDevice(device_id));
    lg_lstm_wide_actor *a = new lg_lstm_wide_actor();
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
    if (hipFuncSetAttribute((const void *)lg::k_lstm_wide_actor, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lg::wide_actor_lds_bytes(512)) != hipSuccess ||
        hipMalloc(&a->d_p, at * sizeof(float)) != hipSuccess || hipMalloc(&a->d_std, 16 * sizeof(float)) != hipSuccess ||
        hipMemset(a->d_p, 0, at * sizeof(float)) != hipSuccess || hipMemset(a->d_std, 0, 16 * sizeof(float)) != hipSuccess) {
        if (a->d_p) (void)hipFree(a->d_p);
        if (a->d_std) (void)hipFree(a->d_std);
        delete a;
        return lg::refuse(-10, "lg_lstm_wide_actor_create: device allocation failed");
    }
    *out = a;
    return 0;
}

int lg_lstm_wide_actor_load_device(lg_lstm_wide_actor *a, const float *const weights[4], const float *const biases[4], const float *std, void *stream) {
    if (!a || !weights || !biases || !std) return lg::refuse(-1, "lg_lstm_wide_actor_load_device: null argument");
    for (int i = 0; i < 4; i++) if (!weights[i] || !biases[i]) return lg::refuse(-1, "lg_lstm_wide_actor_load_device: null layer");
    for (int i = 0; i < 4; i++) {
        const int total = a->pad[i + 1] * a->dims[i] + a->pad[i + 1];
        hipLaunchKernelGGL(lg::k_lstm_wide_actor_pack, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, weights[i], biases[i],
                           a->d_p + a->w_off[i], a->d_p + a->b_off[i], a->dims[i], a->dims[i + 1], a->pad[i + 1]);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(a->d_std, std, a->dims[4] * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

int lg_lstm_wide_actor_destroy(lg_lstm_wide_actor *a) {
    if (!a) return lg::refuse(-1, "lg_lstm_wide_actor_destroy: null handle");
    (void)hipFree(a->d_p);
    (void)hipFree(a->d_std);
    delete a;
    return 0;
}

int lg_lstm_wide_actor_act(const lg_lstm_wide_actor *a, const float *h, float *actions, float *mean, int32_t num_envs, uint64_t seed, int64_t step,
                           const int64_t *step_counter, int32_t deterministic, void *stream) {
    if (!a || !h || !actions) return lg::refuse(-1, "lg_lstm_wide_actor_act: null argument");
    if (num_envs < 1) return lg::refuse(-2, "lg_lstm_wide_actor_act: num_envs must be >= 1");
    lg::LstmActorArgs A = {};
    A.h = h; A.p = a->d_p; A.std = a->d_std; A.actions = actions; A.mean = mean; A.step_counter = step_counter;
    A.seed = seed; A.step = step; A.num_envs = num_envs; A.deterministic = deterministic; A.max_width = a->max_width;
    for (int i = 0; i < 5; i++) { A.dims[i] = a->dims[i]; A.pad[i] = a->pad[i]; }
    for (int i = 0; i < 4; i++) { A.w_off[i] = (uint32_t)a->w_off[i]; A.b_off[i] = (uint32_t)a->b_off[i]; }
    hipLaunchKernelGGL(lg::k_lstm_wide_actor, dim3((num_envs + 31) / 32), dim3(64 * LG_LSTM_WIDE_ACTOR_WAVES), lg::wide_actor_lds_bytes(a->max_width),
                       (hipStream_t)stream, A);
    HIP_TRY(hipGetLastError());
    return 0;
}

const char *lg_lstm_wide_last_error(void) { return lg::g_error; }

}  // extern "C"
