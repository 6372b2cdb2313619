"""NumPy float32 restatement of the decentralised game kernels (csrc/lg_dec_game.hip): ``pre`` = k_dec_pre (the clip block of
DecHighLevelGame.step), ``post`` = k_dec_post (counters, predator integration, termination, both rewards, the predicated reset with the
joints, both observations, the episode means).

Written like tests/game_twin.py, whose pieces it imports: every expression in the kernel's operation order, rounding once per operation,
so everything copied, added, subtracted or multiplied is bit-comparable with the device; values behind ``sqrt`` / ``acos`` (the rewards'
distance, the flags) are not, which is why the tests keep their inputs away from the thresholds (``game_twin.margins``; the decisions AT
the thresholds are pinned against float64 on designed inputs by tests/game_edges.py).  The episode
means are a sum over envs whose order neither torch nor the device fixes: ``means_bound`` is their tolerance."""
import numpy as np

from tests import philox_np as ph
from tests.game_twin import F, GAME_PREDATOR, GAME_ROOT, integrate_predator as _integrate6, norm2, norm3, reset_root, sense, urange, wrap_to_pi  # noqa: F401
from tests.game_twin import assert_margins, margins  # noqa: F401

GAME_DOF = 18
NUM_DOF = 12
SUMS = ("evasion", "pursuit", "termination")          # rows of episode_sums / entries of episode_means


def params(**kw):
    """The fields of lg_dec_game_params with the registered task's values; keyword arguments override.  ``env_radius`` is not a field: it is
    -1 so that game_twin.margins skips the radius check the decentralised game does not have."""
    p = dict(num_envs=0, decimation=4, heading_command=1, custom_origins=0, only_positive_rewards_prey=1, only_positive_rewards_pred=0,
             max_episode_length=1000, seed=1,
             cmd_lin_vel_x=(-1.0, 1.0), cmd_lin_vel_y=(-1.0, 1.0), predator_lin_vel_x=(-2.0, 2.0), predator_lin_vel_y=(-2.0, 2.0),
             capture_dist=0.5, half_fov=1.20428 / 2.0, max_rel_pos=100.0, ll_rew_weight=2.0,
             scale_evasion_dt=0.9 * 0.02, scale_pursuit_dt=0.9 * 0.02, scale_termination_prey_dt=0.0, sim_dt=0.005, predator_z=0.3,
             max_episode_length_s=20.0, base_init_state=(0.0, 0.0, 0.42, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
             default_dof_pos=(0.1, 0.8, -1.5, -0.1, 0.8, -1.5, 0.1, 1.0, -1.5, -0.1, 1.0, -1.5), env_radius=-1.0)
    p.update(kw)
    return p


def _clip(x, r):
    return np.minimum(np.maximum(x, F(r[0])), F(r[1]))


def pre(p, command_prey, command_pred):
    """-> (clipped prey command [N,4], clipped predator command [N,2], low-level commands [N,4])."""
    c, d = np.array(command_prey, F, copy=True), np.array(command_pred, F, copy=True)
    c[:, 0] = _clip(c[:, 0], p["cmd_lin_vel_x"])
    c[:, 1] = _clip(c[:, 1], p["cmd_lin_vel_y"])
    if p["heading_command"]:
        c[:, 2] = wrap_to_pi(c[:, 2])
    d[:, 0] = _clip(d[:, 0], p["predator_lin_vel_x"])
    d[:, 1] = _clip(d[:, 1], p["predator_lin_vel_y"])
    return c, d, c.copy()


def draws(seed, num_envs, step):
    """The uniforms k_dec_post draws for every env: (root [N,8], predator [N,4]) as k_game_post, joints [N,12] (joint j = lane j & 3 of block j >> 2)."""
    e = np.arange(num_envs)
    return ph.lanes(seed, e, step, GAME_ROOT, 0, 8), ph.lanes(seed, e, step, GAME_PREDATOR, 0, 4), ph.lanes(seed, e, step, GAME_DOF, 0, NUM_DOF)


def integrate_predator(p, predator_pos, command_pred):
    n = predator_pos.shape[0]
    c6 = np.zeros((n, 6), F)
    c6[:, 4:6] = command_pred
    return _integrate6(p, predator_pos, c6)


def rewards(p, predator_pos, prey_pos, ll_rew, episode_sums, capture, time_out):
    """-> (rew_prey [N], rew_pred [N], episode_sums [3,N], d [N])."""
    r = (predator_pos - prey_pos).astype(F)
    d = norm3(r[:, 0], r[:, 1], r[:, 2])
    ev, pu = (d * F(p["scale_evasion_dt"])).astype(F), ((-d) * F(p["scale_pursuit_dt"])).astype(F)
    sums = np.array(episode_sums, F, copy=True)
    rew = (F(p["ll_rew_weight"]) * ll_rew.astype(F)).astype(F)
    rew = (rew + ev).astype(F)
    sums[0] = (sums[0] + ev).astype(F)
    if p["only_positive_rewards_prey"]:
        rew = np.maximum(rew, F(0))
    if p["scale_termination_prey_dt"] != 0:
        te = (((capture | time_out) & ~time_out).astype(F) * F(p["scale_termination_prey_dt"])).astype(F)
        rew = (rew + te).astype(F)
        sums[2] = (sums[2] + te).astype(F)
    rp = (F(0) + pu).astype(F)
    sums[1] = (sums[1] + pu).astype(F)
    if p["only_positive_rewards_pred"]:
        rp = np.maximum(rp, F(0))
    return rew, rp, sums, d


def reset_dofs(p, u_dof):
    """LowLevelGame._reset_dofs for every env -> (dof_pos [N,12], dof_vel [N,12])."""
    q = (np.asarray(p["default_dof_pos"], F)[None, :] * urange(0.5, 1.5, u_dof)).astype(F)
    return q, np.zeros_like(q)


def post(p, s, step=None, u_root=None, u_pred=None, u_dof=None):
    """k_dec_post on a state dict ``s`` (command_pred, root_states, dof_pos, dof_vel, env_origins, ll_rew, ll_reset, predator_pos, obs_prey,
    curr_episode_step, episode_length_buf, episode_sums [3,N], episode_means [3]) -> (new state dict incl. obs_pred / rew_prey / rew_pred /
    reset_buf / time_out_buf, info dict with the threshold quantities and ``means_sums`` = the sums the means were formed from)."""
    N = s["root_states"].shape[0]
    if u_root is None:
        u_root, u_pred, u_dof = draws(p["seed"], N, step)
    out = {k: np.array(v, copy=True) for k, v in s.items()}
    root = out["root_states"]
    ep_len = out["episode_length_buf"] + 1
    ep_step = out["curr_episode_step"] + 1
    pp = integrate_predator(p, s["predator_pos"], s["command_pred"])
    info = {"predator_integrated": pp.copy()}
    dist = norm2(root[:, 0] - pp[:, 0], root[:, 1] - pp[:, 1])
    capture = dist < F(p["capture_dist"])
    time_out = ep_len > int(p["max_episode_length"])
    rew_prey, rew_pred, sums, d = rewards(p, pp, root[:, :3], s["ll_rew"], s["episode_sums"], capture, time_out)
    done = capture | time_out | (np.asarray(s["ll_reset"]) != 0)
    info.update(capture=capture, time_out=time_out, done=done, dist_xy=dist, reward_dist=d, means_sums=sums[:, done].copy())
    means = np.array(s["episode_means"], F, copy=True)
    if done.any():
        for i in range(3):
            means[i] = F(F(F(sums[i, done].astype(np.float64).sum()) / F(done.sum())) / F(p["max_episode_length_s"]))
    sums[:, done] = 0
    q, qd = reset_dofs(p, u_dof)
    out["dof_pos"][done], out["dof_vel"][done] = q[done], qd[done]
    r_root, r_pred = reset_root(p, s["env_origins"], u_root, u_pred)
    root[done] = r_root[done]
    pp[done] = r_pred[done]
    obs = np.array(s["obs_prey"], F, copy=True)
    obs[done, 0:12] = F(p["max_rel_pos"])
    obs[done, 12:16] = 0
    ep_len[done] = 0
    ep_step[done] = 0
    sensed, visible, angle, rel, nrel = sense(p, pp, root[:, :3], root[:, 3:7], obs[:, 9:12])
    new_obs = np.concatenate((obs[:, 3:12], sensed, obs[:, 13:16], visible[:, None].astype(F)), axis=1).astype(F)
    info.update(visible=visible, angle=angle, rel_norm=nrel)
    out.update(root_states=root, predator_pos=pp, obs_prey=new_obs, obs_pred=(root[:, :3] - pp).astype(F), rew_prey=rew_prey, rew_pred=rew_pred, reset_buf=done,
               time_out_buf=time_out, curr_episode_step=ep_step, episode_length_buf=ep_len, episode_sums=sums, episode_means=means)
    return out, info


def means_bound(p, info):
    """Tolerance of the three episode means [3].  A mean is (sum of n float32 terms) / n / max_episode_length_s; summing n terms in any order
    and grouping, in float32, is within (n - 1) * 2^-24 * sum|x_i| of the exact sum (the standard bound for recursive summation), and the
    two divisions and the final rounding add 3 * 2^-24 relative.  Nothing here comes from a measured difference."""
    x = info["means_sums"].astype(np.float64)
    n = x.shape[1]
    if n == 0:
        return np.zeros(3)
    return (n + 2) * 2.0 ** -24 * np.abs(x).sum(axis=1) / n / float(p["max_episode_length_s"])
