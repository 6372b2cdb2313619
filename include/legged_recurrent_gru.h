/*
 * legged_recurrent_gru.h -- C-ABI of the GRU cell of a recurrent policy (liblegged_gru.so; the runner key `device_gru`).
 *
 * legged_recurrent.h's cell is an LSTM.  This one advances the two GRU memories of an ActorCriticRecurrent(rnn_type='gru') by one rollout
 * step in one launch, with that cell's launch shape, staged [x | h_in] block and lane maps:
 *
 *     r  = sigma(W_ir x + b_ir + W_hr h + b_hr)
 *     z  = sigma(W_iz x + b_iz + W_hz h + b_hz)
 *     n  = tanh(W_in x + b_in + r * (W_hn h + b_hn))
 *     h' = (1 - z) * n + z * h
 *
 * The x part and the h part of n are separate accumulators (b_hn is inside the product with r), so a wave keeps (r, z, n_x, n_h) of its
 * 32 units where the LSTM keeps (i, f, g, o).  Exact f32 on the matrix cores, each accumulator one k-ordered chain: a row's result depends
 * neither on the launch's width nor on which other role shares the launch.  A saturated z = 1 returns h bit for bit, z = 0 returns n.
 * A policy step is then
 *
 *     lg_gru_step (both memories, one launch) -> lg_lstm_actor_act (legged_recurrent.h) on the actor memory's h
 *
 * One layer; 1 <= num_in <= 256 and hidden a multiple of 32 with 32 <= hidden <= 256.
 *
 * A library of its own: it links against nothing of liblegged_hip.so and its handles are not that library's.  extern "C", 0 = success,
 * negative = error; the text comes from lg_gru_last_error() (per thread), not from lg_last_error().
 */
#ifndef LEGGED_RECURRENT_GRU_H
#define LEGGED_RECURRENT_GRU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LG_GRU_MAX_IN 256
#define LG_GRU_MAX_HIDDEN 256
#define LG_GRU_BLOCK_ENVS 32                      /* env rows per workgroup */

typedef struct lg_gru lg_gru;                     /* opaque; owns the packed weights on the device */

/* HOST arrays in torch.nn.GRU layout: w_ih [3 hidden, num_in], w_hh [3 hidden, hidden], b_ih / b_hh [3 hidden], gate order r, z, n
 * (synchronous: not allowed inside a stream capture).  Raises the kernel's dynamic LDS limit for the device (67 584 B at 256 + 256).
 * Errors, found before anything touches the device: -1 a null argument, -4 an unsupported shape.  -10 a HIP failure. */
int lg_gru_create(int32_t num_in, int32_t hidden, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                  int32_t device_id, lg_gru **out);
/* The same four tensors from DEVICE memory (contiguous float32): one pack launch on `stream`, capture-safe; the operands are the same
 * bits lg_gru_create leaves.  -1 for a null argument. */
int lg_gru_load_device(lg_gru *l, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, void *stream);
int lg_gru_destroy(lg_gru *l);                    /* -1 for a null handle */

/* One launch advances the actor memory (l_a) and the critic memory (l_c) on num_envs rows.  Either role may be absent (a null handle,
 * whose buffers are ignored and which writes nothing).  All buffers are DEVICE, contiguous float32: x_* [num_envs, num_in of the role],
 * h_* [num_envs, hidden of the role].  reset: [num_envs] bytes or NULL; a row whose flag is non-zero starts from h = 0 whatever h_in holds.
 * h_out must not alias h_in of the same role: -2.
 * Errors, all found before anything is launched: -1 both handles null or a null buffer of a present role, -2 num_envs < 1, aliasing or
 * two devices, -10 a HIP failure of the launch. */
int lg_gru_step(const lg_gru *l_a, const lg_gru *l_c, const float *x_a, const float *x_c, const uint8_t *reset,
                const float *h_in_a, float *h_out_a, const float *h_in_c, float *h_out_c, int32_t num_envs, void *stream);

const char *lg_gru_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
