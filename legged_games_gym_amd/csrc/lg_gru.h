// lg_gru.h -- the layout of a GRU cell's handle (include/legged_recurrent_gru.h: lg_gru).  lg_gru.hip (liblegged_gru.so) makes and owns the
// handles; lg_dec_gru.hip (liblegged_dec_game_gru.so) reads them.  Both are compiled from this header by one build.
#pragma once
#include <stdint.h>

struct lg_gru {
    int32_t num_in, hidden, ksteps, device;
    float  *d_wp, *d_bp;
};
static_assert(sizeof(lg_gru) == 32, "lg_gru: four int32 and two device pointers (lg_dec_game_gru_sizeof(0) reports it to the binding)");
