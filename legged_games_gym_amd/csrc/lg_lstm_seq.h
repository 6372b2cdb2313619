// lg_lstm_seq.h -- the LSTM recurrence of the PPO update (include/legged_lstm_sequence.h): handle, kernel arguments, operand layouts.
//
// Both kernels give a workgroup 32 trajectory rows and ALL hidden units, wave w owning units 32 w .. 32 w + 31, for the whole sequence:
// nothing crosses workgroups, so one launch loops over time.  Lane maps are those of the rollout cell (lg_recurrent.h), on
// v_mfma_f32_32x32x2_f32: A lane l = (row l & 31, k = 2 s + (l >> 5)), B lane l = (k = 2 s + (l >> 5), column l & 31), and accumulator
// register r of lane l = (row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31).
//
// k_lstm_seq_fwd: D[row][unit] = bias[unit] + sum_k XH[row][k] W[unit][k], XH = [x_t | h_{t-1}] staged in LDS as xs[k][row] (leading
// dimension 33), W = [W_ih | W_hh] packed as the cell packs it:
//     float4 wp[hidden / 32][ksteps][64], ksteps = (num_in + hidden + 1) / 2: element (w, s, l) = the i, f, g, o weights of unit
//     32 w + (l & 31) at k = 2 s + (l >> 5) (zero at k = K of an odd K);  float4 bp[hidden] = b_ih + b_hh of a unit's four gates.
// The four gate tiles of a wave's units sit in four accumulators, c_t stays in registers from step to step, and h_t goes back into the
// h rows of xs for step t + 1.
//
// k_lstm_seq_bwd: t = T - 1 .. 0.  The elementwise stage turns the saved gates into da (gradient w.r.t. the pre-activations), writes it
// over the gates and into LDS as the A operand da[k = gate hidden + unit][row]; then dh_rec[row][j] = sum_k da[row][k] W_hh[k][j] with
// wave w computing columns j = 32 w .. 32 w + 31: the B operand is row k of torch's W_hh as it lies in memory, and the accumulator's
// register r is again (row, unit l & 31), so dh_rec and dc_rec never leave registers.
#pragma once
#include <stdint.h>

struct lg_lstm_seq {               // (tests/test_lstm_sequence_abi.py mirrors the four leading integers to test the checks without a device)
    int32_t num_in, hidden, ksteps, device;
    float  *d_wp, *d_bp;
};

namespace lg {

#define LG_LSTM_SEQ_LD 33          // floats per k row of a staged [k][row] block

struct LstmSeqFwdArgs {
    const float *x, *h0, *c0, *wp, *bp;
    float *h_out, *gates, *c;      // gates / c: the two blocks of the workspace, both null without one
    int64_t x_step_stride;
    int32_t T, B, num_in, hidden, ksteps, _pad;
};

struct LstmSeqBwdArgs {
    const float *w_hh, *dh_out, *c0, *c;
    float *gates;                  // in: i, f, g, o; out: da_i, da_f, da_g, da_o
    int32_t T, B, hidden, _pad;
};

}  // namespace lg
