"""NumPy float32 restatement of the game kernels (csrc/lg_game.h): ``pre`` = k_game_pre (steps 1-2 of HighLevelGame.step), ``post`` =
k_game_post (episode step, predator integration, reward, dones, root-state reset + predator placement, observation).

Every expression is written in the kernel's operation order and rounds once per operation (the kernels are compiled with floating-point
contraction off), so everything that is copied, added, subtracted or multiplied is bit-comparable with the device; values behind ``sqrt`` /
``acos`` (the reward's distance, the three flags) are not, which is why the tests keep their inputs away from the thresholds (``margins``);
the decisions AT the thresholds are pinned against float64 on designed inputs by tests/game_edges.py.
Draws come from tests/philox_np.py under the two game purposes, or are passed in (fixtures record the draws the reference consumed)."""
import numpy as np

from tests import philox_np as ph

GAME_ROOT, GAME_PREDATOR = 16, 17
F = np.float32
TWO_PI, PI = F(6.2831855), F(3.14159274)


def params(**kw):
    """The fields of lg_game_params with the registered task's values; keyword arguments override."""
    p = dict(num_envs=0, decimation=4, heading_command=1, only_positive_rewards=1, custom_origins=0, seed=1,
             cmd_lin_vel_x=(-1.0, 1.0), cmd_lin_vel_y=(-1.0, 1.0), predator_lin_vel_x=(-2.0, 2.0), predator_lin_vel_y=(-2.0, 2.0),
             capture_dist=0.5, env_radius=-1.0, half_fov=1.20428 / 2.0, max_rel_pos=100.0, ll_rew_weight=2.0,
             scale_evasion_dt=0.9 * 0.02, scale_pursuit_dt=0.9 * 0.02, sim_dt=0.005, predator_z=0.3,
             base_init_state=(0.0, 0.0, 0.42, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0))
    p.update(kw)
    return p


def wrap_to_pi(a):
    a = np.asarray(a, F)
    with np.errstate(invalid="ignore"):
        m = np.fmod(a, TWO_PI).astype(F)
        m = np.where((m != 0) & (m < 0), (m + TWO_PI).astype(F), m)
        return np.where(m > PI, (m - TWO_PI).astype(F), m).astype(F)


def urange(lo, hi, u):
    return ((F(hi) - F(lo)) * u.astype(F) + F(lo)).astype(F)


def pre(p, command):
    """-> (clipped command [N,6], low-level commands [N,4])."""
    c = np.array(command, F, copy=True)
    c[:, 0] = np.minimum(np.maximum(c[:, 0], F(p["cmd_lin_vel_x"][0])), F(p["cmd_lin_vel_x"][1]))
    c[:, 1] = np.minimum(np.maximum(c[:, 1], F(p["cmd_lin_vel_y"][0])), F(p["cmd_lin_vel_y"][1]))
    if p["heading_command"]:
        c[:, 2] = wrap_to_pi(c[:, 2])
    c[:, 4] = np.minimum(np.maximum(c[:, 4], F(p["predator_lin_vel_x"][0])), F(p["predator_lin_vel_x"][1]))
    c[:, 5] = np.minimum(np.maximum(c[:, 5], F(p["predator_lin_vel_y"][0])), F(p["predator_lin_vel_y"][1]))
    return c, c[:, :4].copy()


def draws(seed, num_envs, step):
    """The uniforms k_game_post draws for every env: (root [N,8] = xy offset, 6 velocities; predator [N,4] = 3 offsets, sign)."""
    e = np.arange(num_envs)
    return ph.lanes(seed, e, step, GAME_ROOT, 0, 8), ph.lanes(seed, e, step, GAME_PREDATOR, 0, 4)


def integrate_predator(p, predator_pos, command):
    pp = np.array(predator_pos, F, copy=True)
    dx, dy = (F(p["sim_dt"]) * command[:, 4].astype(F)).astype(F), (F(p["sim_dt"]) * command[:, 5].astype(F)).astype(F)
    for _ in range(int(p["decimation"])):
        pp[:, 0] = (pp[:, 0] + dx).astype(F)
        pp[:, 1] = (pp[:, 1] + dy).astype(F)
    return pp


def norm3(x, y, z):
    return np.sqrt(((x * x).astype(F) + (y * y).astype(F)).astype(F) + (z * z).astype(F)).astype(F)


def norm2(x, y):
    return np.sqrt(((x * x).astype(F) + (y * y).astype(F)).astype(F)).astype(F)


def reward(p, predator_pos, prey_pos, ll_rew, episode_sums):
    """-> (rew [N], episode_sums [2,N], d [N])."""
    r = (predator_pos - prey_pos).astype(F)
    d = norm3(r[:, 0], r[:, 1], r[:, 2])
    ev, pu = (d * F(p["scale_evasion_dt"])).astype(F), ((-d) * F(p["scale_pursuit_dt"])).astype(F)
    rew = (F(p["ll_rew_weight"]) * ll_rew.astype(F)).astype(F)
    rew = (rew + ev).astype(F)
    rew = (rew + pu).astype(F)
    sums = np.array(episode_sums, F, copy=True)
    sums[0] = (sums[0] + ev).astype(F)
    sums[1] = (sums[1] + pu).astype(F)
    if p["only_positive_rewards"]:
        rew = np.maximum(rew, F(0))
    return rew, sums, d


def dones(p, predator_pos, prey_pos, origins, ll_reset):
    """-> dict(capture, radius, done, dist_xy, prey_r, pred_r)."""
    dist = norm2(prey_pos[:, 0] - predator_pos[:, 0], prey_pos[:, 1] - predator_pos[:, 1])
    capture = dist < F(p["capture_dist"])
    prey_r = norm2(prey_pos[:, 0] - origins[:, 0], prey_pos[:, 1] - origins[:, 1])
    pred_r = norm2(predator_pos[:, 0] - origins[:, 0], predator_pos[:, 1] - origins[:, 1])
    radius = np.zeros_like(capture)
    if p["env_radius"] >= 0:
        radius = (prey_r > F(p["env_radius"])) | (pred_r > F(p["env_radius"]))
    return dict(capture=capture, radius=radius, done=capture | radius | (np.asarray(ll_reset) != 0), dist_xy=dist, prey_r=prey_r, pred_r=pred_r)


def reset_root(p, origins, u_root, u_pred):
    """LowLevelGame._reset_root_states for every env -> (root [N,13], predator [N,3])."""
    N = origins.shape[0]
    root = np.tile(np.asarray(p["base_init_state"], F), (N, 1))
    root[:, :3] = (root[:, :3] + origins.astype(F)).astype(F)
    if p["custom_origins"]:
        root[:, 0] = (root[:, 0] + urange(-1.0, 1.0, u_root[:, 0])).astype(F)
        root[:, 1] = (root[:, 1] + urange(-1.0, 1.0, u_root[:, 1])).astype(F)
    root[:, 7:13] = urange(-0.5, 0.5, u_root[:, 2:8])
    sgn = np.where(u_pred[:, 3] < F(0.5), F(-1), F(1)).astype(F)
    pred = np.empty((N, 3), F)
    pred[:, 0] = (root[:, 0] - (sgn * urange(1.0, 10.0, u_pred[:, 0])).astype(F)).astype(F)
    pred[:, 1] = (root[:, 1] - (sgn * urange(1.0, 10.0, u_pred[:, 1])).astype(F)).astype(F)
    pred[:, 2] = F(p["predator_z"])
    return root, pred


def sense(p, predator_pos, prey_pos, quat, newest):
    """sense_predator -> (sensed [N,3], visible [N] bool, angle [N], rel [N,3], |rel| [N])."""
    rel = (predator_pos - prey_pos).astype(F)
    qz, qw = quat[:, 2].astype(F), quat[:, 3].astype(F)
    qn = np.maximum(norm2(qz, qw), F(1e-9))
    yz, yw = (qz / qn).astype(F), (qw / qn).astype(F)
    tz = (yz * F(2)).astype(F)
    fx, fy = (F(1) - (yz * tz).astype(F)).astype(F), (yw * tz).astype(F)
    dot = ((fx * rel[:, 0]).astype(F) + (fy * rel[:, 1]).astype(F)).astype(F)
    nrel = norm3(rel[:, 0], rel[:, 1], rel[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        angle = wrap_to_pi(np.arccos((dot / (norm2(fx, fy) * nrel).astype(F)).astype(F)).astype(F))
        visible = np.abs(angle) <= F(p["half_fov"])
    sensed = np.where(visible[:, None], rel, newest).astype(F)
    return sensed, visible, angle, rel, nrel


def observe(p, obs, predator_pos, prey_pos, quat):
    sensed, visible, angle, rel, nrel = sense(p, predator_pos, prey_pos, quat, obs[:, 9:12])
    new = np.concatenate((obs[:, 3:12], sensed, obs[:, 13:16], visible[:, None].astype(F), (prey_pos - predator_pos).astype(F)), axis=1).astype(F)
    return new, dict(visible=visible, angle=angle, rel_norm=nrel)


def post(p, s, step=None, u_root=None, u_pred=None):
    """k_game_post on a state dict ``s`` (command, root_states, env_origins, ll_rew, ll_reset, predator_pos, obs, curr_episode_step,
    episode_length_buf, episode_sums) -> (new state dict incl. rew / reset_buf, info dict with the threshold quantities)."""
    N = s["root_states"].shape[0]
    if u_root is None:
        u_root, u_pred = draws(p["seed"], N, step)
    out = {k: np.array(v, copy=True) for k, v in s.items()}
    root = out["root_states"]
    ep = out["curr_episode_step"] + 1
    pp = integrate_predator(p, s["predator_pos"], s["command"])
    info = {"predator_integrated": pp.copy()}
    rew, sums, d = reward(p, pp, root[:, :3], s["ll_rew"], s["episode_sums"])
    dn = dones(p, pp, root[:, :3], s["env_origins"], s["ll_reset"])
    done = dn["done"]
    info.update(dn, reward_dist=d)
    r_root, r_pred = reset_root(p, s["env_origins"], u_root, u_pred)
    root[done] = r_root[done]
    pp[done] = r_pred[done]
    obs = np.array(s["obs"], F, copy=True)
    obs[done, 0:12] = F(p["max_rel_pos"])
    obs[done, 12:16] = 0
    obs[done, 16:19] = -F(p["max_rel_pos"])
    ep[done] = 0
    out["episode_length_buf"][done] = 0
    new_obs, oi = observe(p, obs, pp, root[:, :3], root[:, 3:7])
    info.update(oi)
    out.update(root_states=root, predator_pos=pp, obs=new_obs, rew=rew, reset_buf=done, curr_episode_step=ep, episode_sums=sums)
    return out, info


def margins(p, info):
    """Section-3 distances from the thresholds: dict of the smallest |x - threshold| over all envs (inf where a check does not apply)."""
    m = {"angle": float(np.nanmin(np.abs(np.abs(info["angle"]) - F(p["half_fov"])))), "capture": float(np.min(np.abs(info["dist_xy"] - F(p["capture_dist"])))),
         "rel_norm": float(np.min(info["rel_norm"])), "radius": float("inf")}
    if p["env_radius"] >= 0:
        m["radius"] = float(min(np.min(np.abs(info["prey_r"] - F(p["env_radius"]))), np.min(np.abs(info["pred_r"] - F(p["env_radius"])))))
    return m


def assert_margins(p, info):
    m = margins(p, info)
    assert not np.isnan(info["angle"]).any(), "0/0 in the angle"
    assert m["angle"] >= 1e-3 and m["capture"] >= 1e-4 and m["radius"] >= 1e-4 and m["rel_norm"] >= 1e-3, m
    return m
