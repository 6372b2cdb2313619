// lg_game_entry.hip -- the C entry points of the game layers (include/legged_game.h, legged_dec_game.h, legged_pursuer_game.h,
// legged_game_outcome.h, legged_dec_game_outcome.h, legged_dec_game_pool.h, legged_dec_game_member_outcome.h) and the two element-wise
// kernels of lg_game.h, k_game_pre / k_game_post; every other game kernel is a unit of its own behind a launcher.  Each entry header includes what it uses.
#include <hip/hip_runtime.h>

#define LG_POLICY_BLOCKS_ONLY      // lg_policy.h without its two non-template pack kernels (they belong to lg_learner.hip)
#include "lg_game.h"                      // predator-prey game layer: k_game_pre / k_game_post and their entry points
#include "lg_dec_game.h"                  // decentralised game (kernels: lg_dec_game.hip)
#include "lg_pursuer_game.h"              // scripted pursuer (kernel: lg_pursuer_game.hip)
#include "lg_game_outcome_entry.h"        // outcome statistics (kernels: lg_game_outcome.hip)
#include "lg_dec_game_outcome_entry.h"    // decentralised game's outcome statistics (kernel: lg_dec_game_outcome.hip)
#include "lg_dec_game_pool_entry.h"       // decentralised game's opponent pool (kernel: lg_pool_act.hip)
#include "lg_member_outcome_entry.h"      // outcome statistics per pool member (kernel: lg_member_outcome.hip)
