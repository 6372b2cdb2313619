/*
 * legged_lstm_sequence.h -- C-ABI of the LSTM recurrence of a recurrent policy's PPO update: a whole batch of padded trajectories run
 * through time in one launch, forward and backward (back-propagation through time).
 *
 * The rollout advances a memory one step per launch (legged_recurrent.h).  The update evaluates the same memory on [T, B] padded
 * trajectories from their stored initial states and needs the gradients of its four parameter tensors.  Here
 *
 *     lg_lstm_seq_load_device -> lg_lstm_seq_forward -> (MLP, loss and their backward elsewhere) -> lg_lstm_seq_backward
 *
 * run the serial part: forward writes every step's output and, into a workspace, the gates and cell states; backward turns the
 * workspace's gate block into the gradient with respect to the gate pre-activations, dG [T B, 4 hidden].  The caller forms
 * dW_ih = dG^T x, dW_hh = dG^T h_prev and db = column sums of dG with its own GEMMs.
 *
 * The gate GEMM is the rollout cell's: exact f32 on v_mfma_f32_32x32x2_f32, a k-ordered fmaf chain over [x | h] that starts from the
 * bias, and the cell's exp2 / rcp forms of sigma and tanh.  One layer, LSTM only; 1 <= num_in <= 256, hidden a multiple of 32 in
 * 32 .. 256; any T >= 1 and B >= 1.  No atomics: results are bit-identical from run to run.
 *
 * A library of its own (liblegged_lstm_seq.so): extern "C", 0 = success, negative = error, text via lg_lstm_seq_last_error().
 * All buffers are DEVICE memory, contiguous float32 unless a stride is named.
 */
#ifndef LEGGED_LSTM_SEQUENCE_H
#define LEGGED_LSTM_SEQUENCE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LG_LSTM_SEQ_MAX_IN 256
#define LG_LSTM_SEQ_MAX_HIDDEN 256
#define LG_LSTM_SEQ_BLOCK_ROWS 32                 /* trajectory rows per workgroup */

typedef struct lg_lstm_seq lg_lstm_seq;           /* opaque; owns the packed forward operands on the device */

/* Allocates the packed operands (zeros until the first load).  -1 a null `out`, -4 an unsupported shape (both found before anything is
 * allocated), -10 a HIP failure.  Not allowed inside a stream capture. */
int lg_lstm_seq_create(int32_t num_in, int32_t hidden, int32_t device_id, lg_lstm_seq **out);
/* torch.nn.LSTM's tensors (w_ih [4 hidden, num_in], w_hh [4 hidden, hidden], b_ih / b_hh [4 hidden], gate order i, f, g, o) -> the
 * forward's operands: one pack launch on `stream`, capture-safe.  The weights move at every mini-batch, so this runs in front of every
 * forward.  -1 a null argument. */
int lg_lstm_seq_load_device(lg_lstm_seq *s, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, void *stream);
int lg_lstm_seq_destroy(lg_lstm_seq *s);          /* -1 for a null handle */

/* Floats of the workspace of a [T, B] batch: 5 T B hidden (gates [T, B, 4 hidden], then c [T, B, hidden]); 0 for a bad argument. */
size_t lg_lstm_seq_workspace_floats(int32_t T, int32_t B, int32_t hidden);

/* x [T, B, num_in] with x_step_stride floats from step to step (rows inside a step contiguous: a slice of a wider [T, B', num_in]
 * tensor along B'), h0 / c0 [B, hidden] -> h_out [T, B, hidden].  With ws != NULL also ws[0 .. 4 T B hidden) = the post-activation
 * gates as [T, B, 4 hidden] in torch's row order (i, f, g, o blocks of hidden) and ws[4 T B hidden ..) = c as [T, B, hidden];
 * ws == NULL is the forward that needs no gradient and gives the same h_out bit for bit.
 * Errors, all found before the launch: -1 a null argument, -2 T < 1, B < 1, x_step_stride < B num_in, or h_out / ws overlapping an input
 * or each other, -10 a HIP failure of the launch. */
int lg_lstm_seq_forward(const lg_lstm_seq *s, const float *x, int64_t x_step_stride, const float *h0, const float *c0,
                        float *h_out, float *ws, int32_t T, int32_t B, void *stream);

/* dh_out [T, B, hidden]: the gradient with respect to every step's output (zero at padded steps).  ws: what the forward of the same
 * (T, B) left; its gate block is overwritten in place by dG, the gradient with respect to the four gate PRE-activations, same layout.
 * w_hh: torch's own [4 hidden, hidden] tensor (row k is the B operand of dh_prev = dG . W_hh).  c0: the forward's.
 * No gradient is produced for x, h0 or c0.  Errors as above: -1 a null argument, -2 T < 1, B < 1 or ws overlapping an input, -10. */
int lg_lstm_seq_backward(const lg_lstm_seq *s, const float *w_hh, const float *dh_out, const float *c0,
                         float *ws, int32_t T, int32_t B, void *stream);

const char *lg_lstm_seq_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
