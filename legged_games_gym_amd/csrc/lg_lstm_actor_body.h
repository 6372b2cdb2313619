// lg_lstm_actor_body.h -- the actor MLP behind the actor memory of a recurrent policy: the ONE copy of the chain.  k_lstm_actor
// (lg_recurrent.hip, lg_lstm_actor_act) calls it with LG_LSTM_ACTOR_WAVES waves and the stores of that entry point; k_game_lstm_act
// (lg_game_lstm_act.hip, the recurrent high-level role of a game step) with LG_PW_WAVES waves and an epilogue that leaves the means in LDS.
// Needs lg_device.h (rand4, f32x16, LG_DEV) and lg_recurrent.h (LstmActorArgs, LG_LSTM_LD: operand layout and lane maps).
//
// Exact f32 on v_mfma_f32_32x32x2_f32.  An output tile of 32 units is one k-ordered accumulation chain on ONE wave, whichever wave that
// is: the results do not depend on WAVES.
#pragma once

namespace lg {

LG_DEV float lstm_actor_elu(const float x) { return x > 0.0f ? x : (__builtin_amdgcn_exp2f(1.442695041f * x) - 1.0f); }

// The stores of lg_lstm_actor_act: mean (optional) and mean + noise.
//   epilogue(A, env0, row, unit, m, ns)   m = mean of action `unit` (< dims[4]) of row `row` of the workgroup's 32 (any row, live or not);
//                                         ns[row * 16 + unit] = std * eps of that action (0 when deterministic)
struct LstmActorStores {
    LG_DEV void operator()(const LstmActorArgs &A, int env0, int row, int unit, float m, const float *ns) const {
        if (env0 + row < A.num_envs) {
            const size_t at = (size_t)(env0 + row) * A.dims[4] + unit;
            if (A.mean) A.mean[at] = m;
            A.actions[at] = m + ns[row * 16 + unit];
        }
    }
};

// actor(h) of env rows 32 blk .. 32 blk + 31.  Must be called by all WAVES waves of the workgroup (contains barriers; the last statement
// is one).  xa, xb: two activation buffers [max_width][LG_LSTM_LD]; ns: the noise [32][16].  DEPTH: k-steps whose weights a wave requests ahead
// of their products (4 or 16; a k-step count is a multiple of 16), which changes no result.
template <int WAVES, int DEPTH, class Epilogue>
LG_DEV void lstm_actor_body(const LstmActorArgs &A, const int blk, float *xa, float *xb, float *ns, const Epilogue &epilogue) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, env0 = 32 * blk;
    const int nA = A.dims[4];
    {   // the memory's output of the 32 rows as xa[k][row]; rows past num_envs are zeros
        const int H = A.dims[0];
        for (int e = tid; e < 32 * H; e += 64 * WAVES) {
            const int row = e / H, k = e - row * H, env = env0 + row;
            xa[k * LG_LSTM_LD + row] = env < A.num_envs ? A.h[(size_t)env * H + k] : 0.0f;
        }
    }
    if (tid < 128) {                                  // std * eps of actions 4 g .. 4 g + 3 of row tid >> 2 (0 when deterministic)
        const int row = tid >> 2, g = tid & 3, env = env0 + row;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (4 * g < nA && !A.deterministic && env < A.num_envs) {
            const int64_t step = A.step >= 0 ? A.step : (A.step_counter ? A.step_counter[0] + 1 : 0);
            float u[4];
            rand4(A.seed ^ 0x9E3779B97F4A7C15ull, env, step, 100 + g, 0, u);
            const float rad0 = sqrtf(-2.0f * __logf(fmaxf(u[0], 1e-12f))), rad1 = sqrtf(-2.0f * __logf(fmaxf(u[2], 1e-12f)));
            float s0, c0, s1, c1;
            __sincosf(6.2831853f * u[1], &s0, &c0);
            __sincosf(6.2831853f * u[3], &s1, &c1);
            const float eps[4] = {rad0 * c0, rad0 * s0, rad1 * c1, rad1 * s1};
#pragma unroll
            for (int r = 0; r < 4; r++) v[r] = (4 * g + r < nA) ? A.std[4 * g + r] * eps[r] : 0.0f;
        }
#pragma unroll
        for (int r = 0; r < 4; r++) ns[row * 16 + 4 * g + r] = v[r];
    }
    __syncthreads();
#pragma unroll
    for (int L = 0; L < 4; L++) {
        const float *in = (L & 1) ? xb : xa;
        float *out = (L & 1) ? xa : xb;
        const int ks = A.dims[L] / 2, tiles = A.pad[L + 1] / 32;
        const float *al = in + (lane >> 5) * LG_LSTM_LD + (lane & 31);
        for (int o = wave; o < tiles; o += WAVES) {
            const int unit = 32 * o + (lane & 31);
            const float bias = A.p[A.b_off[L] + unit];
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; r++) acc[r] = bias;
            const float *__restrict__ wp = A.p + A.w_off[L] + (size_t)o * ks * 64 + lane;
            if constexpr (DEPTH == 4) {
                for (int s = 0; s < ks; s += 4) {     // (ks is a multiple of 16: the widths are multiples of 32)
                    const float w0 = wp[(size_t)s * 64], w1 = wp[(size_t)(s + 1) * 64], w2 = wp[(size_t)(s + 2) * 64], w3 = wp[(size_t)(s + 3) * 64];
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(al[2 * s * LG_LSTM_LD], w0, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(al[(2 * s + 2) * LG_LSTM_LD], w1, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(al[(2 * s + 4) * LG_LSTM_LD], w2, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(al[(2 * s + 6) * LG_LSTM_LD], w3, acc, 0, 0, 0);
                }
            } else {                                  // the same products in the same order, DEPTH k-steps' operands in flight
                for (int s = 0; s < ks; s += DEPTH) {
                    float w[DEPTH];
#pragma unroll
                    for (int j = 0; j < DEPTH; j++) w[j] = wp[(size_t)(s + j) * 64];
#pragma unroll
                    for (int j = 0; j < DEPTH; j++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(al[2 * (s + j) * LG_LSTM_LD], w[j], acc, 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (L < 3) out[unit * LG_LSTM_LD + row] = lstm_actor_elu(acc[r]);
                else if (unit < nA) epilogue(A, env0, row, unit, acc[r], ns);
            }
        }
        __syncthreads();
    }
}

// One layer of the actor MLP into the packed layout (lg_recurrent.h); one thread per packed weight, then the padded bias: the body of
// k_lstm_actor_pack (lg_recurrent.hip) and k_lstm_wide_actor_pack (lg_lstm_wide.hip).
__device__ __forceinline__ void lstm_actor_pack_body(const float *__restrict__ w, const float *__restrict__ b, float *__restrict__ wp,
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

}  // namespace lg
