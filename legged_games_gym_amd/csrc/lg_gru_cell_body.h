// lg_gru_cell_body.h -- the GRU cell of a recurrent policy's memory (k_gru_cell, lg_gru.hip, lg_gru_step).  Needs lg_device.h (f32x16),
// lg_recurrent.h (LG_LSTM_LD: the staged block and the lane maps are the LSTM cell's) and lg_lstm_cell_body.h (stage_xh: the one copy of the
// staging; lstm_sigmoid, lstm_tanh).
//
// torch's GRU keeps the x part and the h part of the n gate apart (b_hn sits inside the product with r), so a wave's four accumulators
// over the staged [x | h_in] block are (r, z, n_x, n_h): the packed weight of n_x is zero for k >= num_in, that of n_h for k < num_in.
// Exact f32 on v_mfma_f32_32x32x2_f32; each of the four is one k-ordered chain, so a row's result depends neither on the launch's width
// nor on which other role shares it.  A k-step wholly on one side of num_in skips the product whose weight is zero by construction: three
// of four matrix instructions on those k-steps (measured against all four on every k-step: 59.7 against 64.2 us at 2000 envs x 256 units).
#pragma once

namespace lg {

struct GruRole {
    const float *x, *h_in, *wp, *bp;
    float *h_out;
    int32_t num_in, hidden, ksteps, _pad;
};

// k-steps s0 .. s1 - 1 of a wave's chains, four k-steps of operands in flight.  SIDE 0: x only (r, z, n_x), 1: h only (r, z, n_h),
// 2: all four (the k-step that holds the x / h boundary of an odd num_in).
template <int SIDE>
__device__ __forceinline__ void gru_chain(const float4 *__restrict__ wp, const float *xl, int s, const int s1, f32x16 &acc_r, f32x16 &acc_z,
                                          f32x16 &acc_nx, f32x16 &acc_nh) {
#define LG_GRU_KSTEP(W_, A_) \
    acc_r = __builtin_amdgcn_mfma_f32_32x32x2f32(A_, W_.x, acc_r, 0, 0, 0); acc_z = __builtin_amdgcn_mfma_f32_32x32x2f32(A_, W_.y, acc_z, 0, 0, 0); \
    if (SIDE != 1) acc_nx = __builtin_amdgcn_mfma_f32_32x32x2f32(A_, W_.z, acc_nx, 0, 0, 0); \
    if (SIDE != 0) acc_nh = __builtin_amdgcn_mfma_f32_32x32x2f32(A_, W_.w, acc_nh, 0, 0, 0);
    for (; s + 4 <= s1; s += 4) {
        const float4 w0 = wp[(size_t)s * 64], w1 = wp[(size_t)(s + 1) * 64], w2 = wp[(size_t)(s + 2) * 64], w3 = wp[(size_t)(s + 3) * 64];
        const float a0 = xl[2 * s * LG_LSTM_LD], a1 = xl[(2 * s + 2) * LG_LSTM_LD], a2 = xl[(2 * s + 4) * LG_LSTM_LD], a3 = xl[(2 * s + 6) * LG_LSTM_LD];
        LG_GRU_KSTEP(w0, a0) LG_GRU_KSTEP(w1, a1) LG_GRU_KSTEP(w2, a2) LG_GRU_KSTEP(w3, a3)
    }
    for (; s < s1; s++) {
        const float4 w = wp[(size_t)s * 64];
        const float a = xl[2 * s * LG_LSTM_LD];
        LG_GRU_KSTEP(w, a)
    }
#undef LG_GRU_KSTEP
}

// One role's workgroup: env rows 32 blk .. 32 blk + 31, all hidden units (hidden / 32 waves).
__device__ __forceinline__ void gru_cell_role(const GruRole &R, const uint8_t *__restrict__ reset, const int num_envs, const int blk, float *xs) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int I = R.num_in, H = R.hidden;
    const bool active = wave < H / 32;                                            // (the launch is sized for the wider role: the narrower
    const int env0 = 32 * blk;                                                    //  one's surplus waves only meet the barrier)
    if (active) stage_xh(R.x, R.h_in, I, H, reset, num_envs, env0, tid, 2 * H, xs);        // lg_lstm_cell_body.h: 64 threads per 32 hidden units
    __syncthreads();
    if (!active) return;

    const int unit = 32 * wave + (lane & 31);
    const float4 b = ((const float4 *)R.bp)[unit];
    f32x16 acc_r, acc_z, acc_nx, acc_nh;
#pragma unroll
    for (int r = 0; r < 16; r++) { acc_r[r] = b.x; acc_z[r] = b.y; acc_nx[r] = b.z; acc_nh[r] = b.w; }
    const float4 *__restrict__ wp = (const float4 *)R.wp + (size_t)wave * R.ksteps * 64 + lane;
    const float *xl = xs + (lane >> 5) * LG_LSTM_LD + (lane & 31);
    const int sx = I / 2, sh = (I + 1) / 2;       // k-steps below sx hold x only, from sh on h (and the pad) only; an odd I leaves one between
    gru_chain<0>(wp, xl, 0, sx, acc_r, acc_z, acc_nx, acc_nh);
    gru_chain<2>(wp, xl, sx, sh, acc_r, acc_z, acc_nx, acc_nh);
    gru_chain<1>(wp, xl, sh, R.ksteps, acc_r, acc_z, acc_nx, acc_nh);
    // cell update straight from the accumulators: register r is env row (r & 3) + 8 (r >> 2) + 4 (lane >> 5), column = unit.  h' in the form
    // (1 - z) n + z h: a saturated z = 1 returns h_prev and z = 0 returns n, bit for bit
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int env = env0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (env < num_envs) {
            const size_t o = (size_t)env * H + unit;
            const float h_prev = (reset && reset[env]) ? 0.0f : R.h_in[o];
            const float rg = lstm_sigmoid(acc_r[r]), z = lstm_sigmoid(acc_z[r]);
            const float n = lstm_tanh(acc_nx[r] + rg * acc_nh[r]);
            R.h_out[o] = (1.0f - z) * n + z * h_prev;
        }
    }
}

}  // namespace lg
