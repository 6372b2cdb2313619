/*
 * legged_recurrent_wide.h -- C-ABI of the LSTM cell and actor MLP of a recurrent policy whose memories have up to 512 units
 * (liblegged_lstm_wide.so; the runner key `wide_memory`).
 *
 * legged_recurrent.h's cell gives one workgroup all units of a memory and stops at 256.  This one splits the units over workgroups: a
 * workgroup is 32 env rows x one unit group of up to 256 units, every workgroup stages the whole [x | h_in] block of its rows, and wave w of
 * group g runs the k-ordered chain of units 256 g + 32 w .. + 31 -- the same chain, operand layout and epilogue as lg_lstm_step, so at a
 * width both take the results are the same bits.  A policy step is then
 *
 *     lg_lstm_wide_step (both memories, one launch) -> lg_lstm_wide_actor_act on the actor memory's h
 *
 * One layer, LSTM only; 1 <= num_in <= 256 and hidden a multiple of 32 with 32 <= hidden <= 512.
 *
 * A library of its own: it links against nothing of liblegged_hip.so and its handles are not that library's.  extern "C", 0 = success,
 * negative = error; the text comes from lg_lstm_wide_last_error() (per thread), not from lg_last_error().
 */
#ifndef LEGGED_RECURRENT_WIDE_H
#define LEGGED_RECURRENT_WIDE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LG_LSTM_WIDE_MAX_IN 256
#define LG_LSTM_WIDE_MAX_HIDDEN 512
#define LG_LSTM_WIDE_GROUP_UNITS 256              /* units per workgroup */
#define LG_LSTM_WIDE_BLOCK_ENVS 32                /* env rows per workgroup */

typedef struct lg_lstm_wide lg_lstm_wide;         /* opaque; owns the packed weights on the device */

/* HOST arrays in torch.nn.LSTM layout, as lg_lstm_create: w_ih [4 hidden, num_in], w_hh [4 hidden, hidden], b_ih / b_hh [4 hidden], gate
 * order i, f, g, o (synchronous: not allowed inside a stream capture).  Raises the kernel's dynamic LDS limit for the device.
 * Errors, found before anything is allocated: -1 a null argument, -4 an unsupported shape.  -10 a HIP failure. */
int lg_lstm_wide_create(int32_t num_in, int32_t hidden, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                        int32_t device_id, lg_lstm_wide **out);
/* The same four tensors from DEVICE memory (contiguous float32): one pack launch on `stream`, capture-safe; the operands are the same
 * bits lg_lstm_wide_create leaves.  -1 for a null argument. */
int lg_lstm_wide_load_device(lg_lstm_wide *l, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, void *stream);
int lg_lstm_wide_destroy(lg_lstm_wide *l);        /* -1 for a null handle */

/* lg_lstm_step for memories of up to 512 units: one launch advances the actor memory (l_a) and the critic memory (l_c) on num_envs rows.
 * Either role may be absent (a null handle, whose buffers are ignored).  All buffers are DEVICE, contiguous float32: x_* [num_envs, num_in
 * of the role], h_* / c_* [num_envs, hidden of the role].  reset: [num_envs] bytes or NULL; a row whose flag is non-zero starts from a zero
 * (h, c).  h_out / c_out must not alias h_in / c_in of the same role (the other unit group reads them): -2.
 * Errors, all found before anything is launched: -1 both handles null or a null buffer of a present role, -2 num_envs < 1, aliasing or
 * two devices, -10 a HIP failure of the launch. */
int lg_lstm_wide_step(const lg_lstm_wide *l_a, const lg_lstm_wide *l_c, const float *x_a, const float *x_c, const uint8_t *reset,
                      const float *h_in_a, const float *c_in_a, float *h_out_a, float *c_out_a,
                      const float *h_in_c, const float *c_in_c, float *h_out_c, float *c_out_c, int32_t num_envs, void *stream);

/* The actor MLP behind a wide actor memory: lg_lstm_actor_* with dims[0] a multiple of 32 in 32 .. 512; three hidden widths (multiples of
 * 32 in 32 .. 512, ELU), 1 .. 16 actions, the Philox noise stream and the step handling of lg_lstm_actor_act.
 * create allocates only (-1 null argument, -4 unsupported widths, -10 HIP failure; not inside a capture); load_device packs the four
 * layers' torch.nn.Linear tensors and std from DEVICE memory on `stream`, capture-safe, and must run before the first act.
 * act: h [num_envs, dims[0]] -> actions, mean [num_envs, dims[4]] (mean may be NULL); step >= 0, or step < 0 to read step_counter[0] + 1 on
 * the device; deterministic != 0 gives actions = mean.  -1 null argument, -2 num_envs < 1. */
typedef struct lg_lstm_wide_actor lg_lstm_wide_actor;
int lg_lstm_wide_actor_create(const int32_t dims[5], int32_t device_id, lg_lstm_wide_actor **out);
int lg_lstm_wide_actor_load_device(lg_lstm_wide_actor *a, const float *const weights[4], const float *const biases[4], const float *std, void *stream);
int lg_lstm_wide_actor_destroy(lg_lstm_wide_actor *a);
int lg_lstm_wide_actor_act(const lg_lstm_wide_actor *a, const float *h, float *actions, float *mean, int32_t num_envs, uint64_t seed, int64_t step,
                           const int64_t *step_counter, int32_t deterministic, void *stream);

const char *lg_lstm_wide_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
