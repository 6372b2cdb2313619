// lg_lstm_cell_body.h -- the LSTM cell of a recurrent policy's memory: the ONE copy of the staging (stage_xh), of the cell's chain and update
// (lstm_units) and of the weight pack (lstm_pack_body).  k_lstm_cell (lg_recurrent.hip, lg_lstm_step) calls lstm_cell_role for its two
// roles; k_dec_lstm_cell (lg_dec_game_lstm_act.hip, lg_dec_lstm_step) and k_dec_pool_lstm_cell for the up to four memories of a
// decentralised game step; k_lstm_wide_cell (lg_lstm_wide.hip) calls stage_xh and lstm_units with its own split of a memory's units over
// workgroups; gru_cell_role (lg_gru_cell_body.h) calls stage_xh.  Needs lg_device.h (f32x16) and lg_recurrent.h (LstmRole, LG_LSTM_LD:
// operand layout and lane maps).
//
// Exact f32 on v_mfma_f32_32x32x2_f32.  A wave's 32 units are one k-ordered accumulation chain: the results depend neither on the launch's
// width nor on which other roles share it.
#pragma once

namespace lg {

// 1-ulp v_exp_f32 / v_rcp_f32 (the build's fast-math convention): sigma saturates to exactly 0 / 1 and tanh to -1 / 1 through inf
__device__ __forceinline__ float lstm_sigmoid(const float x) { return 1.0f / (1.0f + __builtin_amdgcn_exp2f(-1.44269504088896341f * x)); }
__device__ __forceinline__ float lstm_tanh(const float x) { return 1.0f - 2.0f / (1.0f + __builtin_amdgcn_exp2f(2.88539008177792681f * x)); }

// Stage [x | h_in] of env rows env0 .. env0 + 31 as xs[k][row], by the `nthreads` threads tid = 0 .. nthreads - 1 the caller sends: rows
// past num_envs and the pad row k = K of an odd K (the buffer holds 2 ksteps = K + 1 rows then) are zeros, a reset row's h is zero.  The
// ONE copy of the staging: the LSTM cell, the wide LSTM cell (lg_lstm_wide.hip) and the GRU cell (lg_gru_cell_body.h) call it.
__device__ __forceinline__ void stage_xh(const float *x, const float *h_in, const int I, const int H,
                                         const uint8_t *__restrict__ reset, const int num_envs, const int env0, const int tid, const int nthreads,
                                         float *xs) {
    for (int e = tid; e < 32 * I; e += nthreads) {
        const int row = e / I, k = e - row * I, env = env0 + row;
        xs[k * LG_LSTM_LD + row] = env < num_envs ? x[(size_t)env * I + k] : 0.0f;
    }
    for (int e = tid; e < 32 * H; e += nthreads) {
        const int row = e / H, k = e - row * H, env = env0 + row;
        const bool live = env < num_envs && !(reset && reset[env]);
        xs[(I + k) * LG_LSTM_LD + row] = live ? h_in[(size_t)env * H + k] : 0.0f;
    }
    if (((I + H) & 1) && tid < 32) xs[(I + H) * LG_LSTM_LD + tid] = 0.0f;
}

// The 32 units 32 gw .. 32 gw + 31 of a role on the staged block: bias, the k-ordered chain, the cell update.  The ONE copy of the chain:
// lstm_cell_role sends its wave index, lstm_wide_role (lg_lstm_wide.hip) the wave's index among all unit groups of the memory.
__device__ __forceinline__ void lstm_units(const LstmRole &R, const uint8_t *__restrict__ reset, const int num_envs, const int env0, const int gw,
                                           const int lane, const float *xs) {
    const int H = R.hidden, unit = 32 * gw + (lane & 31);
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
    for (; s + 4 <= R.ksteps; s += 4) {           // four k-steps' operands in flight: 4 KB of weights per wave and trip
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

// One role's workgroup: env rows 32 blk .. 32 blk + 31, all hidden units (hidden / 32 waves, 64 threads per 32 hidden units).  The launch
// is sized for the wider role: the narrower one's surplus waves only meet the barrier.
__device__ __forceinline__ void lstm_cell_role(const LstmRole &R, const uint8_t *__restrict__ reset, const int num_envs, const int blk, float *xs) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool active = wave < R.hidden / 32;
    const int env0 = 32 * blk;
    if (active) stage_xh(R.x, R.h_in, R.num_in, R.hidden, reset, num_envs, env0, tid, 2 * R.hidden, xs);
    __syncthreads();
    if (active) lstm_units(R, reset, num_envs, env0, wave, lane, xs);
}

// [w_ih | w_hh] (torch.nn.LSTM layout, gate order i, f, g, o) -> wp, b_ih + b_hh -> bp (lg_recurrent.h).  One thread per float4 of the
// packed layout: the body of k_lstm_pack (lg_recurrent.hip) and k_lstm_wide_pack (lg_lstm_wide.hip).
__device__ __forceinline__ void lstm_pack_body(const float *__restrict__ w_ih, const float *__restrict__ w_hh, const float *__restrict__ b_ih,
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

}  // namespace lg
