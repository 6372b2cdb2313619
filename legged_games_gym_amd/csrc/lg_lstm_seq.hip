// lg_lstm_seq.hip -- k_lstm_seq_pack / k_lstm_seq_fwd / k_lstm_seq_bwd and their entry points (include/legged_lstm_sequence.h): the LSTM
// recurrence of a recurrent policy's PPO update, a whole padded trajectory batch through time in one launch each way.  Operand layouts
// and lane maps: lg_lstm_seq.h.  The only unit of liblegged_lstm_seq.so: it includes nothing that instantiates a kernel of liblegged_hip.so.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "lg_lstm_seq.h"
#include "../../include/legged_lstm_sequence.h"

namespace lg {

typedef float f32x16 __attribute__((ext_vector_type(16)));

static thread_local char seq_error[256] = "";

static int seq_fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(seq_error, sizeof(seq_error), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(x) do { hipError_t _e = (x); if (_e != hipSuccess) return lg::seq_fail(-10, "HIP error: %s", hipGetErrorString(_e)); } while (0)

// [w_ih | w_hh] (torch.nn.LSTM layout, gate order i, f, g, o) -> wp, b_ih + b_hh -> bp.  One thread per float4 of the packed layout.
__global__ void __launch_bounds__(256) k_lstm_seq_pack(const float *__restrict__ w_ih, const float *__restrict__ w_hh, const float *__restrict__ b_ih,
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

// the rollout cell's forms (1-ulp v_exp_f32 / v_rcp_f32): sigma saturates to exactly 0 / 1 and tanh to -1 / 1 through inf
__device__ __forceinline__ float seq_sigmoid(const float x) { return 1.0f / (1.0f + __builtin_amdgcn_exp2f(-1.44269504088896341f * x)); }
__device__ __forceinline__ float seq_tanh(const float x) { return 1.0f - 2.0f / (1.0f + __builtin_amdgcn_exp2f(2.88539008177792681f * x)); }

// Workgroup b: trajectory rows 32 b .. 32 b + 31, all hidden units (hidden / 32 waves), steps 0 .. T - 1.
__global__ void __launch_bounds__(2 * LG_LSTM_SEQ_MAX_HIDDEN) k_lstm_seq_fwd(const LstmSeqFwdArgs A) {
    extern __shared__ float xs[];                                                 // [2 ksteps][LG_LSTM_SEQ_LD]
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int I = A.num_in, H = A.hidden, K = I + H, B = A.B, nthreads = 2 * H;
    const int row0 = LG_LSTM_SEQ_BLOCK_ROWS * (int)blockIdx.x;
    // h_0 of the 32 rows into the h rows of xs; rows past B and the pad row k = K are zeros for the whole sequence's start
    for (int e = tid; e < 32 * H; e += nthreads) {
        const int row = e / H, k = e - row * H, tr = row0 + row;
        xs[(I + k) * LG_LSTM_SEQ_LD + row] = tr < B ? A.h0[(size_t)tr * H + k] : 0.0f;
    }
    if ((K & 1) && tid < 32) xs[K * LG_LSTM_SEQ_LD + tid] = 0.0f;
    const int unit = 32 * wave + (lane & 31);
    const int rbase = row0 + 4 * (lane >> 5);                                     // register r: row rbase + (r & 3) + 8 (r >> 2)
    float c[16];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int tr = rbase + (r & 3) + 8 * (r >> 2);
        c[r] = tr < B ? A.c0[(size_t)tr * H + unit] : 0.0f;
    }
    const float4 b = ((const float4 *)A.bp)[unit];
    const float4 *__restrict__ wp = (const float4 *)A.wp + (size_t)wave * A.ksteps * 64 + lane;
    const float *xl = xs + (lane >> 5) * LG_LSTM_SEQ_LD + (lane & 31);
    const size_t H4 = (size_t)4 * H;
    // The weights come from L2 at every step, in groups of four k-steps (4 KB per wave); the next group is requested before the current
    // one's 16 MFMAs issue, and the first group of step t + 1 before the epilogue of step t, so a load's latency is spent under matrix work.
    const int groups = A.ksteps / 4;                                              // (>= 4: ksteps >= 17)
    float4 w0 = wp[0], w1 = wp[64], w2 = wp[128], w3 = wp[192];
    // staging of x_t: this thread's elements are tid, tid + nthreads, ...; (row, k) of the first and the step from one to the next
    const int n_x = 32 * I, n_live = (int)min((int64_t)n_x, (int64_t)(B - row0) * I);   // elements of rows below B; the rest are zeros
    const int x_row = tid / I, x_k = tid - x_row * I, x_drow = nthreads / I, x_dk = nthreads - x_drow * I;

    for (int t = 0; t < A.T; t++) {
        // 1. x_t next to the h_{t-1} already staged (every wave is past the second barrier of step t - 1: nobody reads the x rows)
        // (the block's 32 rows are one run of 32 I floats of x_t: element e of it is (row e / I, k e % I); eight loads in flight per thread)
        const float *__restrict__ xb = A.x + (size_t)t * A.x_step_stride + (size_t)row0 * I;
        for (int e0 = tid, row = x_row, k = x_k; e0 < n_x; e0 += 8 * nthreads) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; j++) v[j] = e0 + j * nthreads < n_live ? xb[e0 + j * nthreads] : 0.0f;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                if (e0 + j * nthreads < n_x) xs[k * LG_LSTM_SEQ_LD + row] = v[j];
                k += x_dk; row += x_drow;
                if (k >= I) { k -= I; row++; }
            }
        }
        __syncthreads();
        // 2. the gate GEMM: bias first, then k-ordered over [x | h]
        f32x16 acc_i, acc_f, acc_g, acc_o;
#pragma unroll
        for (int r = 0; r < 16; r++) { acc_i[r] = b.x; acc_f[r] = b.y; acc_g[r] = b.z; acc_o[r] = b.w; }
#define LG_SEQ_KSTEP(W_, A_) \
        acc_i = __builtin_amdgcn_mfma_f32_32x32x2f32(A_, W_.x, acc_i, 0, 0, 0); acc_f = __builtin_amdgcn_mfma_f32_32x32x2f32(A_, W_.y, acc_f, 0, 0, 0); \
        acc_g = __builtin_amdgcn_mfma_f32_32x32x2f32(A_, W_.z, acc_g, 0, 0, 0); acc_o = __builtin_amdgcn_mfma_f32_32x32x2f32(A_, W_.w, acc_o, 0, 0, 0);
        for (int g = 0; g < groups; g++) {
            const int s = 4 * g, sn = g + 1 < groups ? s + 4 : 0;                 // (behind the last group: the first one, for step t + 1)
            const float4 n0 = wp[(size_t)sn * 64], n1 = wp[(size_t)(sn + 1) * 64], n2 = wp[(size_t)(sn + 2) * 64], n3 = wp[(size_t)(sn + 3) * 64];
            const float a0 = xl[2 * s * LG_LSTM_SEQ_LD], a1 = xl[(2 * s + 2) * LG_LSTM_SEQ_LD], a2 = xl[(2 * s + 4) * LG_LSTM_SEQ_LD], a3 = xl[(2 * s + 6) * LG_LSTM_SEQ_LD];
            LG_SEQ_KSTEP(w0, a0) LG_SEQ_KSTEP(w1, a1) LG_SEQ_KSTEP(w2, a2) LG_SEQ_KSTEP(w3, a3)
            w0 = n0; w1 = n1; w2 = n2; w3 = n3;
        }
        for (int s = 4 * groups; s < A.ksteps; s++) {
            const float4 w = wp[(size_t)s * 64];
            const float a = xl[2 * s * LG_LSTM_SEQ_LD];
            LG_SEQ_KSTEP(w, a)
        }
#undef LG_SEQ_KSTEP
        __syncthreads();                                                          // every wave has read the old h rows
        // 3. - 5. the cell update from the accumulators; gates, c_t, h_t to global memory; h_t into the h rows for step t + 1
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = 4 * (lane >> 5) + (r & 3) + 8 * (r >> 2), tr = row0 + row;
            const float gi = seq_sigmoid(acc_i[r]), gf = seq_sigmoid(acc_f[r]), gg = seq_tanh(acc_g[r]), go = seq_sigmoid(acc_o[r]);
            const float cn = gf * c[r] + gi * gg;
            const float hn = go * seq_tanh(cn);
            c[r] = cn;
            xs[(I + unit) * LG_LSTM_SEQ_LD + row] = hn;
            if (tr < B) {
                const size_t at = (size_t)t * B + tr;
                A.h_out[at * H + unit] = hn;
                if (A.gates) {
                    float *g = A.gates + at * H4 + unit;
                    g[0] = gi; g[H] = gf; g[2 * H] = gg; g[3 * H] = go;
                    A.c[at * H + unit] = cn;
                }
            }
        }
    }
}

// Same ownership, steps T - 1 .. 0.
__global__ void __launch_bounds__(2 * LG_LSTM_SEQ_MAX_HIDDEN) k_lstm_seq_bwd(const LstmSeqBwdArgs A) {
    extern __shared__ float da[];                                                 // [4 hidden][LG_LSTM_SEQ_LD]: the A operand [k][row]
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = A.hidden, B = A.B;
    const int row0 = LG_LSTM_SEQ_BLOCK_ROWS * (int)blockIdx.x;
    const int unit = 32 * wave + (lane & 31);
    const size_t H4 = (size_t)4 * H;
    f32x16 dh_rec;
    float dc_rec[16], ct[16];                                                     // ct: c_t of the step about to run
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int tr = row0 + 4 * (lane >> 5) + (r & 3) + 8 * (r >> 2);
        dh_rec[r] = 0.0f; dc_rec[r] = 0.0f;
        ct[r] = tr < B ? A.c[((size_t)(A.T - 1) * B + tr) * H + unit] : 0.0f;
    }
    const float *__restrict__ wl = A.w_hh + (size_t)(lane >> 5) * H + unit;       // W_hh[k + (lane >> 5)][unit]: + k H per k
    const float *al = da + (lane >> 5) * LG_LSTM_SEQ_LD + (lane & 31);
    // W_hh comes from L2 at every step, in groups of 32 k rows (one float per lane and MFMA); the next group is requested before the
    // current one's 16 MFMAs issue, and the first group of step t - 1 under the last of step t.
    float w[16];
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = wl[(size_t)(2 * j) * H];

    for (int t = A.T - 1; t >= 0; t--) {
        // elementwise: (row, unit) of register r is what the accumulator of the previous step's GEMM holds.
        // Eight registers at a time, all of their loads first: the gates are overwritten in place, and a store between two loads orders
        // them (16 round trips to memory per step instead of 2).  c_{t-1} is loaded here and kept: it is step t - 1's c_t.
#pragma unroll
        for (int half = 0; half < 2; half++) {
            float gi[8], gf[8], gg[8], go[8], cp[8], dho[8];
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int r = 8 * half + j, tr = row0 + 4 * (lane >> 5) + (r & 3) + 8 * (r >> 2);
                gi[j] = gf[j] = gg[j] = go[j] = cp[j] = dho[j] = 0.0f;
                if (tr < B) {
                    const size_t at = (size_t)t * B + tr;
                    const float *g = A.gates + at * H4 + unit;
                    gi[j] = g[0]; gf[j] = g[H]; gg[j] = g[2 * H]; go[j] = g[3 * H];
                    cp[j] = t > 0 ? A.c[(at - B) * H + unit] : A.c0[(size_t)tr * H + unit];
                    dho[j] = A.dh_out[at * H + unit];
                }
            }
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int r = 8 * half + j, row = 4 * (lane >> 5) + (r & 3) + 8 * (r >> 2), tr = row0 + row;
                float da_i = 0.0f, da_f = 0.0f, da_g = 0.0f, da_o = 0.0f;
                if (tr < B) {
                    float *g = A.gates + ((size_t)t * B + tr) * H4 + unit;
                    const float dh = dho[j] + dh_rec[r];
                    const float tc = seq_tanh(ct[r]);
                    const float dc = dc_rec[r] + dh * go[j] * (1.0f - tc * tc);
                    da_o = dh * tc * (go[j] * (1.0f - go[j]));
                    da_i = dc * gg[j] * (gi[j] * (1.0f - gi[j]));
                    da_f = dc * cp[j] * (gf[j] * (1.0f - gf[j]));
                    da_g = dc * gi[j] * (1.0f - gg[j] * gg[j]);
                    dc_rec[r] = dc * gf[j];
                    ct[r] = cp[j];
                    g[0] = da_i; g[H] = da_f; g[2 * H] = da_g; g[3 * H] = da_o;
                }
                da[(unit) * LG_LSTM_SEQ_LD + row] = da_i;
                da[(H + unit) * LG_LSTM_SEQ_LD + row] = da_f;
                da[(2 * H + unit) * LG_LSTM_SEQ_LD + row] = da_g;
                da[(3 * H + unit) * LG_LSTM_SEQ_LD + row] = da_o;
            }
        }
        if (t == 0) break;                                                        // dh_0 is asked of nobody
        __syncthreads();
        // dh_rec[row][unit] = sum_k da[row][k] W_hh[k][unit], k = 0 .. 4 hidden - 1 in order
#pragma unroll
        for (int r = 0; r < 16; r++) dh_rec[r] = 0.0f;
        for (int k = 0; k < 4 * H; k += 32) {                                     // (4 hidden is a multiple of 128)
            const int kn = k + 32 < 4 * H ? k + 32 : 0;                           // (behind the last group: the first one, for step t - 1)
            float wn[16], a[16];
#pragma unroll
            for (int j = 0; j < 16; j++) wn[j] = wl[(size_t)(kn + 2 * j) * H];
#pragma unroll
            for (int j = 0; j < 16; j++) a[j] = al[(k + 2 * j) * LG_LSTM_SEQ_LD];
#pragma unroll
            for (int j = 0; j < 16; j++) dh_rec = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], w[j], dh_rec, 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 16; j++) w[j] = wn[j];
        }
        __syncthreads();                                                          // every wave has read da before step t - 1 overwrites it
    }
}

static size_t fwd_lds_bytes(const int ksteps) { return (size_t)2 * ksteps * LG_LSTM_SEQ_LD * sizeof(float); }
static size_t bwd_lds_bytes(const int hidden) { return (size_t)4 * hidden * LG_LSTM_SEQ_LD * sizeof(float); }

// [a, a + na) and [b, b + nb) floats share an address
static bool overlap(const float *a, size_t na, const float *b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + na * sizeof(float), b0 = (uintptr_t)b, b1 = b0 + nb * sizeof(float);
    return a0 < b1 && b0 < a1;
}

}  // namespace lg

extern "C" {

const char *lg_lstm_seq_last_error(void) { return lg::seq_error; }

int lg_lstm_seq_create(int32_t num_in, int32_t hidden, int32_t device_id, lg_lstm_seq **out) {
    if (!out) return lg::seq_fail(-1, "lg_lstm_seq_create: null argument");
    *out = nullptr;
    if (num_in < 1 || num_in > LG_LSTM_SEQ_MAX_IN)
        return lg::seq_fail(-4, "lg_lstm_seq_create: num_in must be 1 .. 256");
    if (hidden < 32 || hidden > LG_LSTM_SEQ_MAX_HIDDEN || hidden % 32)
        return lg::seq_fail(-4, "lg_lstm_seq_create: hidden must be a multiple of 32 in 32 .. 256 (one layer, LSTM only)");
    HIP_TRY(hipSetDevice(device_id));
    // both staged blocks of the largest shape are above the 64 KB a kernel gets without asking
    HIP_TRY(hipFuncSetAttribute((const void *)lg::k_lstm_seq_fwd, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lg::fwd_lds_bytes((LG_LSTM_SEQ_MAX_IN + LG_LSTM_SEQ_MAX_HIDDEN) / 2)));
    HIP_TRY(hipFuncSetAttribute((const void *)lg::k_lstm_seq_bwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lg::bwd_lds_bytes(LG_LSTM_SEQ_MAX_HIDDEN)));
    lg_lstm_seq *s = new lg_lstm_seq();
    s->num_in = num_in; s->hidden = hidden; s->ksteps = (num_in + hidden + 1) / 2; s->device = device_id;
    s->d_wp = s->d_bp = nullptr;
    const size_t n_wp = (size_t)(hidden / 32) * s->ksteps * 64 * 4, n_bp = (size_t)4 * hidden;
    if (hipMalloc(&s->d_wp, n_wp * sizeof(float)) != hipSuccess || hipMalloc(&s->d_bp, n_bp * sizeof(float)) != hipSuccess ||
        hipMemset(s->d_wp, 0, n_wp * sizeof(float)) != hipSuccess || hipMemset(s->d_bp, 0, n_bp * sizeof(float)) != hipSuccess) {
        if (s->d_wp) (void)hipFree(s->d_wp);
        if (s->d_bp) (void)hipFree(s->d_bp);
        delete s;
        return lg::seq_fail(-10, "lg_lstm_seq_create: device allocation failed");
    }
    *out = s;
    return 0;
}

int lg_lstm_seq_load_device(lg_lstm_seq *s, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, void *stream) {
    if (!s || !w_ih || !w_hh || !b_ih || !b_hh) return lg::seq_fail(-1, "lg_lstm_seq_load_device: null argument");
    const int total = (s->hidden / 32) * s->ksteps * 64 + s->hidden;
    hipLaunchKernelGGL(lg::k_lstm_seq_pack, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, w_ih, w_hh, b_ih, b_hh,
                       (float4 *)s->d_wp, (float4 *)s->d_bp, s->num_in, s->hidden, s->ksteps);
    HIP_TRY(hipGetLastError());
    return 0;
}

int lg_lstm_seq_destroy(lg_lstm_seq *s) {
    if (!s) return lg::seq_fail(-1, "lg_lstm_seq_destroy: null handle");
    (void)hipFree(s->d_wp);
    (void)hipFree(s->d_bp);
    delete s;
    return 0;
}

size_t lg_lstm_seq_workspace_floats(int32_t T, int32_t B, int32_t hidden) {
    if (T < 1 || B < 1 || hidden < 1) return 0;
    return (size_t)5 * (size_t)T * (size_t)B * (size_t)hidden;
}

int lg_lstm_seq_forward(const lg_lstm_seq *s, const float *x, int64_t x_step_stride, const float *h0, const float *c0,
                        float *h_out, float *ws, int32_t T, int32_t B, void *stream) {
    if (!s || !x || !h0 || !c0 || !h_out) return lg::seq_fail(-1, "lg_lstm_seq_forward: null argument");
    if (T < 1 || B < 1) return lg::seq_fail(-2, "lg_lstm_seq_forward: T and B must be >= 1");
    const size_t I = (size_t)s->num_in, H = (size_t)s->hidden, TB = (size_t)T * (size_t)B;
    if (x_step_stride < (int64_t)((size_t)B * I)) return lg::seq_fail(-2, "lg_lstm_seq_forward: x_step_stride is smaller than B num_in");
    const size_t n_x = (size_t)(T - 1) * (size_t)x_step_stride + (size_t)B * I, n_state = (size_t)B * H, n_out = TB * H, n_ws = 5 * TB * H;
    if (lg::overlap(h_out, n_out, x, n_x) || lg::overlap(h_out, n_out, h0, n_state) || lg::overlap(h_out, n_out, c0, n_state) ||
        (ws && (lg::overlap(ws, n_ws, x, n_x) || lg::overlap(ws, n_ws, h0, n_state) || lg::overlap(ws, n_ws, c0, n_state) || lg::overlap(ws, n_ws, h_out, n_out))))
        return lg::seq_fail(-2, "lg_lstm_seq_forward: h_out / ws must not alias an input or each other");
    lg::LstmSeqFwdArgs A = {};
    A.x = x; A.h0 = h0; A.c0 = c0; A.wp = s->d_wp; A.bp = s->d_bp; A.h_out = h_out;
    A.gates = ws; A.c = ws ? ws + 4 * TB * H : nullptr;
    A.x_step_stride = x_step_stride; A.T = T; A.B = B; A.num_in = s->num_in; A.hidden = s->hidden; A.ksteps = s->ksteps;
    const int blocks = (B + LG_LSTM_SEQ_BLOCK_ROWS - 1) / LG_LSTM_SEQ_BLOCK_ROWS;
    hipLaunchKernelGGL(lg::k_lstm_seq_fwd, dim3(blocks), dim3(2 * s->hidden), lg::fwd_lds_bytes(s->ksteps), (hipStream_t)stream, A);
    HIP_TRY(hipGetLastError());
    return 0;
}

int lg_lstm_seq_backward(const lg_lstm_seq *s, const float *w_hh, const float *dh_out, const float *c0,
                         float *ws, int32_t T, int32_t B, void *stream) {
    if (!s || !w_hh || !dh_out || !c0 || !ws) return lg::seq_fail(-1, "lg_lstm_seq_backward: null argument");
    if (T < 1 || B < 1) return lg::seq_fail(-2, "lg_lstm_seq_backward: T and B must be >= 1");
    const size_t H = (size_t)s->hidden, TB = (size_t)T * (size_t)B, n_ws = 5 * TB * H;
    if (lg::overlap(ws, n_ws, w_hh, 4 * H * H) || lg::overlap(ws, n_ws, dh_out, TB * H) || lg::overlap(ws, n_ws, c0, (size_t)B * H))
        return lg::seq_fail(-2, "lg_lstm_seq_backward: ws must not alias an input");
    lg::LstmSeqBwdArgs A = {};
    A.w_hh = w_hh; A.dh_out = dh_out; A.c0 = c0; A.gates = ws; A.c = ws + 4 * TB * H;
    A.T = T; A.B = B; A.hidden = s->hidden;
    const int blocks = (B + LG_LSTM_SEQ_BLOCK_ROWS - 1) / LG_LSTM_SEQ_BLOCK_ROWS;
    hipLaunchKernelGGL(lg::k_lstm_seq_bwd, dim3(blocks), dim3(2 * s->hidden), lg::bwd_lds_bytes(s->hidden), (hipStream_t)stream, A);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
