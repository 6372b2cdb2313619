// lg_dec_game_post.h -- one env of the post stage of the decentralised predator-prey game: dec_post_env<OUTCOME>, the body of k_dec_post
// (lg_dec_game.hip, OUTCOME = false) and of k_dec_outcome (lg_dec_game_outcome.hip, OUTCOME = true), so that everything the two kernels
// write per env comes out bit-identical.  Device code only; needs lg_device.h.
#pragma once
#include "lg_game_post.h"      // the integrator, the root reset and the observation writer of the post stage
#include "../../include/legged_dec_game.h"

namespace lg {

enum { RNG_GAME_DOF = 18 };      // Philox purpose of the joint reset; root and predator: RNG_GAME_ROOT / RNG_GAME_PREDATOR (lg_game_post.h)
#define LG_DEC_BLOCK 256
#define LG_DEC_WAVES (LG_DEC_BLOCK / 64)
inline dim3 dec_grid(const lg_dec_game_params &P) { return dim3((P.num_envs + LG_DEC_BLOCK - 1) / LG_DEC_BLOCK); }      // one thread per env

// One env of post_physics_step (:236-258).  red = (1, evasion sum, pursuit sum, termination sum) of a done env as the sums stood before
// zeroing (:301-305), untouched otherwise.
// OUTCOME: returns the flags of a done env as bits 0..4 (done, captured, timed_out, fell, ll_timed_out), 0 for an env that goes on, and
// `*steps` receives the episode's length in high-level steps (done envs only); without it the result is 0 and `ll_time_out_buf` and
// `steps` are not touched.
template <bool OUTCOME>
LG_DEV unsigned dec_post_env(const lg_dec_game_params &P, const lg_dec_game_buffers &B, const uint8_t *ll_time_out_buf, const int e, const int64_t step,
                             float (&red)[4], unsigned long long *steps) {
#pragma clang fp contract(off)
    const size_t N = (size_t)P.num_envs;
    float *root = B.ll_root_states + (size_t)e * 13;
    float *pp = B.predator_pos + (size_t)e * 3;
    float *obs = B.obs_prey + (size_t)e * LG_DEC_NUM_OBS_PREY;
    const float *org = B.ll_env_origins + (size_t)e * 3;

    int64_t ep_len = B.episode_length_buf[e] + 1;                                             // (:243)
    int64_t ep_step = B.curr_episode_step[e] + 1;                                             // (:244)

    // step_predator_single_integrator (:228-230)
    GamePose s = game_load_pose(pp, root);
    game_integrate_predator(P.sim_dt, P.decimation, B.command_pred[(size_t)e * LG_DEC_NUM_ACTIONS_PRED],
                            B.command_pred[(size_t)e * LG_DEC_NUM_ACTIONS_PRED + 1], s);

    // check_termination (:263-269)
    const float ax = s.qx - s.px, ay = s.qy - s.py;
    const bool capture = sqrtf(ax * ax + ay * ay) < P.capture_dist;
    const bool time_out = ep_len > (int64_t)P.max_episode_length;
    bool done = capture || time_out;

    // compute_reward_prey (:321-341), compute_reward_pred (:344-361)
    float sum_ev = B.episode_sums[e], sum_pu = B.episode_sums[N + e], sum_te = B.episode_sums[2 * N + e];
    {
        const float rx = s.px - s.qx, ry = s.py - s.qy, rz = s.pz - s.qz;
        const float d = sqrtf((rx * rx + ry * ry) + rz * rz);
        const float ev = d * P.scale_evasion_dt, pu = (-d) * P.scale_pursuit_dt;
        float rew = P.ll_rew_weight * B.ll_rew_buf[e];
        rew = rew + ev;
        sum_ev = sum_ev + ev;
        if (P.only_positive_rewards_prey) rew = fmaxf(rew, 0.0f);
        if (P.scale_termination_prey_dt != 0.0f) {                                            // after the clip; reset_buf * ~time_out_buf BEFORE the low-level resets join
            const float te = ((done && !time_out) ? 1.0f : 0.0f) * P.scale_termination_prey_dt;
            rew = rew + te;
            sum_te = sum_te + te;
        }
        B.rew_prey[e] = rew;
        float rp = 0.0f + pu;
        sum_pu = sum_pu + pu;
        if (P.only_positive_rewards_pred) rp = fmaxf(rp, 0.0f);
        B.rew_pred[e] = rp;
    }
    done = done || B.ll_reset_buf[e] != 0;                                                    // (:252)

    unsigned flags = 0;
    GameHistory k;
    k.load(obs);
    if (done) {
        red[0] = 1.0f; red[1] = sum_ev; red[2] = sum_pu; red[3] = sum_te;                     // (:300-305)
        sum_ev = 0.0f; sum_pu = 0.0f; sum_te = 0.0f;
        if constexpr (OUTCOME) {
            const bool ll_reset = B.ll_reset_buf[e] != 0, ll_time_out = ll_time_out_buf[e] != 0;
            flags = 1u | (capture ? 2u : 0u) | (time_out ? 4u : 0u) | ((ll_reset && !ll_time_out) ? 8u : 0u) | ((ll_reset && ll_time_out) ? 16u : 0u);
            *steps = (unsigned long long)ep_step;
        }
        // LowLevelGame._reset_dofs (low_level_game.py:391-392): joint j draws lane j & 3 of block j >> 2
        float2 *ds = reinterpret_cast<float2 *>(B.ll_dof_state) + (size_t)e * LG_DEC_NUM_DOF;
#pragma unroll
        for (int b = 0; b < LG_DEC_NUM_DOF / 4; b++) {
            float uj[4];
            rand4(P.seed, e, step, RNG_GAME_DOF, b, uj);
#pragma unroll
            for (int l = 0; l < 4; l++) ds[4 * b + l] = make_float2(P.default_dof_pos[4 * b + l] * game_urange(0.5f, 1.5f, uj[l]), 0.0f);
        }
        game_reset_root(P, e, step, org, root, s);
        k.clear(P.max_rel_pos);                                                               // DecHighLevelGame.reset_idx (:291-296)
        ep_len = 0;
        ep_step = 0;
    }
    B.episode_length_buf[e] = ep_len;
    B.curr_episode_step[e] = ep_step;
    B.reset_buf[e] = done ? 1 : 0;
    B.time_out_buf[e] = time_out ? 1 : 0;
    B.episode_sums[e] = sum_ev; B.episode_sums[N + e] = sum_pu; B.episode_sums[2 * N + e] = sum_te;
    pp[0] = s.px; pp[1] = s.py; pp[2] = s.pz;

    // compute_observations_pred (:389-391), prey_sense_predator (:417-448) + compute_observations_prey (:374-380)
    float *op = B.obs_pred + (size_t)e * LG_DEC_NUM_OBS_PRED;
    op[0] = s.qx - s.px; op[1] = s.qy - s.py; op[2] = s.qz - s.pz;
    game_observe(P.half_fov, s, k, obs);
    return flags;
}

}  // namespace lg
