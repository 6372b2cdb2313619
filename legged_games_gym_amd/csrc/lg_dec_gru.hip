// lg_dec_gru.hip -- k_dec_gru_cell / lg_dec_gru_step (include/legged_dec_game_gru.h): the GRU memories of both agents of a decentralised
// game step (predator actor / critic, prey actor / critic) advanced in one launch, workgroups split by role.  A role is a call of
// gru_cell_role (lg_gru_cell_body.h), the call k_gru_cell (lg_gru.hip) makes: the same bits.  The GRU twin of k_dec_lstm_cell
// (lg_dec_game_lstm_act.hip).
// The only translation unit of liblegged_dec_game_gru.so: it links against nothing of the other libraries.  The layout of the handles
// liblegged_gru.so created comes from lg_gru.h, which both are compiled from.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lg_device.h"             // f32x16
#include "lg_recurrent.h"          // LG_LSTM_LD: the staged block and the lane maps
#include "lg_lstm_cell_body.h"     // stage_xh, lstm_sigmoid, lstm_tanh
#include "lg_gru_cell_body.h"
#include "lg_gru.h"                // struct lg_gru
#include "lg_lib_error.h"          // g_error, refuse, raise_lds_limit, HIP_TRY_WHO
#include "../../include/legged_dec_game_gru.h"

namespace lg {

struct DecGruArgs {
    GruRole role[4];               // predator actor / critic memory, prey actor / critic memory; only the present ones are filled
    const uint8_t *reset;
    int32_t num_envs, blocks;      // workgroups per present role
    uint32_t order, _pad;          // two bits per slot: the role of workgroups slot * blocks .. (slot + 1) * blocks - 1
};

__global__ void __launch_bounds__(2 * LG_GRU_MAX_HIDDEN) k_dec_gru_cell(const DecGruArgs A) {
    extern __shared__ float xs[];                                                 // [2 ksteps of the largest present role][LG_LSTM_LD]
    const int slot = (int)blockIdx.x / A.blocks, blk = (int)blockIdx.x - slot * A.blocks;
    switch ((A.order >> (2 * slot)) & 3u) {                                       // (a constant index each: the arguments stay where they are)
        case 0: gru_cell_role(A.role[0], A.reset, A.num_envs, blk, xs); break;
        case 1: gru_cell_role(A.role[1], A.reset, A.num_envs, blk, xs); break;
        case 2: gru_cell_role(A.role[2], A.reset, A.num_envs, blk, xs); break;
        default: gru_cell_role(A.role[3], A.reset, A.num_envs, blk, xs); break;
    }
}

static size_t gru_lds_bytes(const int ksteps) { return (size_t)2 * ksteps * LG_LSTM_LD * sizeof(float); }
static const int GRU_MAX_KSTEPS = (LG_GRU_MAX_IN + LG_GRU_MAX_HIDDEN) / 2;

}  // namespace lg

extern "C" {

int lg_dec_gru_step(const lg_dec_gru_role roles[4], const uint8_t *reset, int32_t num_envs, void *stream) {
    static const char *const who = "lg_dec_gru_step";
    static const char *const names[4] = {"predator actor", "predator critic", "prey actor", "prey critic"};
    if (!roles) return lg::refuse(-1, "%s: null roles", who);
    int present = 0, hidden = 0, ksteps = 0, device = 0;
    for (int r = 0; r < 4; r++) {
        const lg_dec_gru_role &R = roles[r];
        if (!R.l) continue;
        if (!R.x || !R.h_in || !R.h_out) return lg::refuse(-1, "%s: null buffer of the %s memory", who, names[r]);
        present++;
    }
    if (!present) return lg::refuse(-1, "%s: all four handles are null", who);
    if (num_envs < 1) return lg::refuse(-2, "%s: num_envs must be >= 1", who);
    lg::DecGruArgs A = {};
    int slot = 0;
    for (int r = 0; r < 4; r++) {
        const lg_dec_gru_role &R = roles[r];
        if (!R.l) continue;
        if (R.h_out == R.h_in)
            return lg::refuse(-2, "%s: h_out of the %s memory must not alias h_in (the epilogue reads h_in while other waves write h_out)", who, names[r]);
        if (slot && R.l->device != device) return lg::refuse(-2, "%s: the memories live on different devices", who);
        device = R.l->device;
        lg::GruRole &K = A.role[r];
        K.x = R.x; K.h_in = R.h_in; K.h_out = R.h_out;
        K.wp = R.l->d_wp; K.bp = R.l->d_bp; K.num_in = R.l->num_in; K.hidden = R.l->hidden; K.ksteps = R.l->ksteps;
        if (K.hidden > hidden) hidden = K.hidden;
        if (K.ksteps > ksteps) ksteps = K.ksteps;
        A.order |= (uint32_t)r << (2 * slot++);
    }
    // the block size and the staged block come from the handles: nothing outside what lg_gru_create makes reaches the launch
    for (int r = 0; r < 4; r++) {
        const lg::GruRole &K = A.role[r];
        if (!roles[r].l) continue;
        if (K.num_in < 1 || K.num_in > LG_GRU_MAX_IN || K.hidden < 32 || K.hidden > LG_GRU_MAX_HIDDEN || K.hidden % 32 || K.ksteps != (K.num_in + K.hidden + 1) / 2)
            return lg::refuse(-2, "%s: the shape of the %s memory's handle is outside what lg_gru_create makes", who, names[r]);
    }
    static bool raised[64] = {};
    HIP_TRY_WHO(lg::raise_lds_limit((const void *)lg::k_dec_gru_cell, lg::gru_lds_bytes(lg::GRU_MAX_KSTEPS), raised));
    A.reset = reset;
    A.num_envs = num_envs;
    A.blocks = (num_envs + LG_GRU_BLOCK_ENVS - 1) / LG_GRU_BLOCK_ENVS;
    hipLaunchKernelGGL(lg::k_dec_gru_cell, dim3(present * A.blocks), dim3(2 * hidden), lg::gru_lds_bytes(ksteps), (hipStream_t)stream, A);
    HIP_TRY_WHO(hipGetLastError());
    return 0;
}

const char *lg_dec_game_gru_last_error(void) { return lg::g_error; }

int lg_dec_game_gru_sizeof(int which) {
    switch (which) {
        case 0: return (int)sizeof(lg_gru);
        case 1: return (int)sizeof(lg_dec_gru_role);
        default: return -1;
    }
}

}  // extern "C"
