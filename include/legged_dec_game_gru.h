/*
 * legged_dec_game_gru.h -- C-ABI of the shared cell launch of GRU policies on the decentralised predator-prey game (task
 * `dec_high_level_game`; the runner key `dec_gru_shared` on top of `device_gru`): the GRU memories of both agents advanced in one launch.
 *
 * legged_dec_game_recurrent.h's cell launch reads lg_lstm handles.  This one is its twin for the lg_gru handles of liblegged_gru.so
 * (legged_recurrent_gru.h).  The actor MLP behind a GRU memory is the main library's lg_lstm_actor and reads only h, so the actor launch
 * of that header serves unchanged, and the policy stage of a step with two GRU agents is two launches,
 *     lg_dec_gru_step (up to four memories)  ->  lg_dec_game_lstm_act  ->  lg_step  ->  lg_dec_game_post / lg_dec_outcome_post
 * where the entry points of legged_recurrent_gru.h and legged_recurrent.h need six (lg_gru_step x 2, lg_lstm_actor_act x 2,
 * lg_dec_game_pre, lg_policy_act).
 *
 * A library of its own, liblegged_dec_game_gru.so: it links against nothing of the other libraries and reads the handles liblegged_gru.so
 * created; both are built by one build from the same headers.  extern "C", stateless, raw device pointers owned by the caller,
 * 0 = success, negative = error with the text in lg_dec_game_gru_last_error() (this library's own, per thread).
 * The first call on a device raises the kernel's dynamic LDS limit (67 584 B at 256 + 256, as lg_gru_create does for its kernel): make it
 * outside any stream capture.
 */
#ifndef LEGGED_DEC_GAME_GRU_H
#define LEGGED_DEC_GAME_GRU_H

#include <stdint.h>
#include "legged_recurrent_gru.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One memory of the cell launch: lg_gru_step's arguments of one role.  x [N, num_in of l], h_in / h_out [N, hidden of l], DEVICE,
 * contiguous float32.  l == NULL: the role is absent, its pointers are ignored and it writes nothing. */
typedef struct lg_dec_gru_role {
    const lg_gru *l;
    const float  *x, *h_in;
    float        *h_out;
} lg_dec_gru_role;

/* One launch advances up to four memories by one step on num_envs rows, workgroups split by role:
 *   roles[0] predator actor memory, roles[1] predator critic memory, roles[2] prey actor memory, roles[3] prey critic memory.
 * Each present role's h_out is bit-identical to lg_gru_step with that role alone.  reset: [num_envs] bytes or NULL, shared by the roles;
 * a row whose flag is non-zero starts from h = 0.  h_out must not alias h_in of the same role.  No atomics: the same bits on every run.
 * Errors, all found before anything is launched: -1 `roles` null, no present role or a null buffer of a present role; -2 num_envs < 1,
 * aliasing, or memories on different devices; -10 a HIP failure. */
int lg_dec_gru_step(const lg_dec_gru_role roles[4], const uint8_t *reset, int32_t num_envs, void *stream);

/* the text of this thread's last error of this library */
const char *lg_dec_game_gru_last_error(void);

/* sizeof as this library sees them of 0: lg_gru, 1: lg_dec_gru_role; -1 otherwise */
int lg_dec_game_gru_sizeof(int which);

#ifdef __cplusplus
}
#endif
#endif
