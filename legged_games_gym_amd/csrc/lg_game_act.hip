// lg_game_act.hip -- the translation unit of k_prey_act (lg_game_act.h).  The kernel is built from the blocks of lg_policy.h; it is compiled
// apart from lg_kernels.hip so that the code hipcc generates for the kernels there does not depend on it (see lg_game.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#define LG_POLICY_BLOCKS_ONLY      // lg_policy.h without its two non-template pack kernels (they belong to lg_learner.hip)
#include "lg_device.h"
#include "lg_policy.h"
#include "lg_game_act.h"
