// lg_dec_game_privileged.hip -- k_privileged_obs / lg_dec_game_privileged_obs (include/legged_dec_game_privileged.h): the critic-only
// observations of the decentralised predator-prey game, one launch behind whichever post kernel ran (k_dec_post, k_dec_outcome,
// k_member_outcome).  Those three sit at their amdgpu_num_sgpr(96) cap with their by-value arguments; two more pointers in each would be
// three more twins to keep bit-identical, so the writer is a launch of its own that leaves every other kernel as it is.
// The only translation unit of liblegged_dec_game_privileged.so: it links against nothing of the other libraries.
//
// Floating point: contraction is OFF in the body, every expression rounds once per operation in the order written.  Copies, p - q and the
// clock (game_quotient: correctly rounded) are bit-comparable with the NumPy twin (tests/dec_privileged_twin.py); fx, fy sit behind
// sqrtf and the fast division (1 ulp and 2.5 ulp on this build).
#include <hip/hip_runtime.h>
#include <stdint.h>

#define LG_POLICY_BLOCKS_ONLY      // lg_policy.h (which lg_game_common.h needs) without its two non-template pack kernels
#include "lg_device.h"
#include "lg_policy.h"
#include "lg_dec_game_post.h"      // LG_DEC_BLOCK, dec_grid; game_quotient (lg_game_post.h)
#include "lg_lib_error.h"          // g_error, refuse, HIP_TRY_WHO
#include "../../include/legged_dec_game_privileged.h"

namespace lg {

// what the kernel reads of the two structs: a kernel argument segment of 64 bytes instead of their 400
struct PrivilegedArgs {
    const float *predator_pos, *root_states, *obs_prey, *obs_pred;
    const int64_t *episode_length_buf;
    float *priv_pred, *priv_prey;
    int32_t num_envs, max_episode_length;
};

__global__ __launch_bounds__(LG_DEC_BLOCK) void k_privileged_obs(const PrivilegedArgs A) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * LG_DEC_BLOCK + threadIdx.x;
    if (e >= A.num_envs) return;
    const float *root = A.root_states + (size_t)e * 13;
    const float *oy = A.obs_prey + (size_t)e * LG_DEC_NUM_OBS_PREY;
    // the yaw-forward vector, the lines of game_observe (lg_game_post.h): quat_apply_yaw, then quat_apply(q_yaw, (1, 0, 0))
    const float quat_z = root[5], quat_w = root[6];
    const float qn = fmaxf(sqrtf(quat_z * quat_z + quat_w * quat_w), 1e-9f);
    const float yz = quat_z / qn, yw = quat_w / qn;
    const float tz = yz * 2.0f;
    const float fx = 1.0f - yz * tz, fy = yw * tz;
    const float L = (float)A.max_episode_length;
    const float clock = game_quotient(L - (float)A.episode_length_buf[e], L);                // no clamp
    if (A.priv_prey) {
        const float *pp = A.predator_pos + (size_t)e * 3;
        float *d = A.priv_prey + (size_t)e * LG_DEC_NUM_PRIV_PREY;
#pragma unroll
        for (int i = 0; i < LG_DEC_NUM_OBS_PREY; i++) d[i] = oy[i];
        d[16] = pp[0] - root[0]; d[17] = pp[1] - root[1]; d[18] = pp[2] - root[2];           // rx, ry, rz of game_observe
        d[19] = fx; d[20] = fy;
        d[21] = clock;
    }
    if (A.priv_pred) {
        const float *op = A.obs_pred + (size_t)e * LG_DEC_NUM_OBS_PRED;
        float *d = A.priv_pred + (size_t)e * LG_DEC_NUM_PRIV_PRED;
        d[0] = op[0]; d[1] = op[1]; d[2] = op[2];
        d[3] = fx; d[4] = fy;
        d[5] = root[7]; d[6] = root[8]; d[7] = root[9];
        d[8] = oy[15];
        d[9] = clock;
    }
}

}  // namespace lg

extern "C" {

int lg_dec_game_privileged_obs(const lg_dec_game_params *P, const lg_dec_game_buffers *B, float *priv_pred, float *priv_prey, void *stream) {
    static const char *const who = "lg_dec_game_privileged_obs";
    if (!P || !B) return lg::refuse(-1, "%s: null argument", who);
    if (!priv_pred && !priv_prey) return lg::refuse(-1, "%s: both destinations are null", who);
    if (!B->predator_pos || !B->ll_root_states || !B->obs_prey || !B->episode_length_buf || (priv_pred && !B->obs_pred))
        return lg::refuse(-1, "%s: null predator_pos, ll_root_states, obs_prey, obs_pred or episode_length_buf in the buffers", who);
    if (P->num_envs < 1) return lg::refuse(-2, "%s: num_envs must be >= 1", who);
    if (P->max_episode_length < 1) return lg::refuse(-2, "%s: max_episode_length must be >= 1", who);
    const lg::PrivilegedArgs A = {B->predator_pos, B->ll_root_states, B->obs_prey, B->obs_pred, B->episode_length_buf, priv_pred, priv_prey,
                                  P->num_envs, P->max_episode_length};
    hipLaunchKernelGGL(lg::k_privileged_obs, lg::dec_grid(*P), dim3(LG_DEC_BLOCK), 0, (hipStream_t)stream, A);
    HIP_TRY_WHO(hipGetLastError());
    return 0;
}

const char *lg_dec_game_privileged_last_error(void) { return lg::g_error; }

int lg_dec_game_privileged_sizeof(int which) {
    switch (which) {
        case 0: return (int)sizeof(lg_dec_game_params);
        case 1: return (int)sizeof(lg_dec_game_buffers);
        default: return -1;
    }
}

}  // extern "C"
