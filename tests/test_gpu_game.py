"""-m gpu: the predator-prey game layer -- ``lg_game_pre`` / ``lg_game_post`` against the NumPy twin and the reference's recorded step,
``HighLevelGame.step`` against its parts, known answers (pursuit time, reset placement, occlusion, radius), the captured step against
eager steps, and the registry / runner / play surface.  Nothing here reads the reference tree: what is needed lies in tests/golden/."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import game_twin as tw
from tests.game_fixtures import check_call, game_registered, load, sequence_calls, synthetic_state  # noqa: F401

pytestmark = pytest.mark.gpu
F = np.float32
DEV = "cuda:0"


# ----------------------------------------------------------------------------- kernels without an env
def pack_params(p):
    from legged_games_gym_amd import capi
    P = capi.lg_game_params()
    for k in ("num_envs", "decimation", "heading_command", "only_positive_rewards", "custom_origins", "seed"):
        setattr(P, k, int(p[k]))
    for k in ("cmd_lin_vel_x", "cmd_lin_vel_y", "predator_lin_vel_x", "predator_lin_vel_y", "base_init_state"):
        capi._fill(getattr(P, k), p[k])
    for k in ("capture_dist", "env_radius", "half_fov", "max_rel_pos", "ll_rew_weight", "scale_evasion_dt", "scale_pursuit_dt", "sim_dt", "predator_z"):
        setattr(P, k, float(p[k]))
    return P


def unpack_params(P):
    p = {k: int(getattr(P, k)) for k in ("num_envs", "decimation", "heading_command", "only_positive_rewards", "custom_origins", "seed")}
    p.update({k: tuple(float(v) for v in getattr(P, k)) for k in ("cmd_lin_vel_x", "cmd_lin_vel_y", "predator_lin_vel_x", "predator_lin_vel_y", "base_init_state")})
    p.update({k: float(getattr(P, k)) for k in ("capture_dist", "env_radius", "half_fov", "max_rel_pos", "ll_rew_weight", "scale_evasion_dt", "scale_pursuit_dt", "sim_dt",
                                                "predator_z")})
    return p


def device_pre(p, command):
    from legged_games_gym_amd import capi
    n = command.shape[0]
    c = torch.from_numpy(np.ascontiguousarray(command, F)).to(DEV)
    ll = torch.full((n, 4), 7.0, device=DEV)
    capi.game_pre(pack_params(dict(p, num_envs=n)), capi.game_buffers({"command": c.data_ptr(), "ll_commands": ll.data_ptr()}), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return c.cpu().numpy(), ll.cpu().numpy()


def device_post(p, s, step, counter_on_device=False):
    """``lg_game_post`` on the arrays of a twin state dict, uploaded as they are -> the same dict layout as ``game_twin.post`` returns."""
    from legged_games_gym_amd import capi
    n = s["root_states"].shape[0]
    t = {k: torch.from_numpy(np.ascontiguousarray(s[k])).to(DEV) for k in ("command", "root_states", "env_origins", "ll_rew", "predator_pos", "obs", "curr_episode_step",
                                                                           "episode_length_buf", "episode_sums")}
    t["ll_reset"] = torch.from_numpy(np.ascontiguousarray(s["ll_reset"]).astype(bool)).to(DEV)
    t["rew"], t["reset_buf"] = torch.full((n,), -3.0, device=DEV), torch.zeros(n, dtype=torch.bool, device=DEV)
    t["counter"] = torch.tensor([step], dtype=torch.int64, device=DEV)
    for k in ("command", "root_states", "env_origins", "ll_rew", "predator_pos", "obs", "episode_sums"):
        assert t[k].dtype == torch.float32
    B = capi.game_buffers({"command": t["command"].data_ptr(), "ll_root_states": t["root_states"].data_ptr(), "ll_env_origins": t["env_origins"].data_ptr(),
                           "ll_rew_buf": t["ll_rew"].data_ptr(), "ll_reset_buf": t["ll_reset"].data_ptr(), "ll_step_counter": t["counter"].data_ptr(),
                           "predator_pos": t["predator_pos"].data_ptr(), "obs": t["obs"].data_ptr(), "rew": t["rew"].data_ptr(), "reset_buf": t["reset_buf"].data_ptr(),
                           "curr_episode_step": t["curr_episode_step"].data_ptr(), "episode_length_buf": t["episode_length_buf"].data_ptr(),
                           "episode_sums": t["episode_sums"].data_ptr()})
    capi.game_post(pack_params(dict(p, num_envs=n)), B, -1 if counter_on_device else step, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = {k: t[k].cpu().numpy() for k in ("root_states", "predator_pos", "obs", "rew", "reset_buf", "curr_episode_step", "episode_length_buf", "episode_sums")}
    assert int(t["counter"][0]) == step and np.array_equal(t["command"].cpu().numpy(), s["command"])          # inputs are left alone
    return out


@pytest.mark.parametrize("tag", ["a", "b"])
def test_kernels_reproduce_the_recorded_reference_step(golden_dir, tag):
    """game_step.npz through the DEVICE: the state is carried by the device's own outputs; same comparison as tests/test_game_reference.py,
    with 2 more ulp on the floats behind the device's 1-ulp sqrt."""
    g = load(golden_dir, "game_step.npz")
    p = json.loads(str(g[f"{tag}_params"]))
    state = {k: g[f"{tag}_in0_{k}"] for k in ("predator_pos", "obs", "curr_episode_step", "episode_length_buf", "episode_sums")}
    state["env_origins"] = g[f"{tag}_env_origins"]
    for k in range(g[f"{tag}_step"].shape[0]):
        command, ll_cmd = device_pre(p, g[f"{tag}_in_command"][k])
        want_cmd = g[f"{tag}_command"][k]
        np.testing.assert_array_equal(command.view(np.uint32), want_cmd.view(np.uint32))
        np.testing.assert_array_equal(ll_cmd.view(np.uint32), want_cmd[:, :4].view(np.uint32))
        s = dict(state, command=command, root_states=g[f"{tag}_in_root_states"][k], ll_rew=g[f"{tag}_in_ll_rew"][k], ll_reset=g[f"{tag}_in_ll_dones"][k])
        _, info = tw.post(p, s, u_root=g[f"{tag}_u_root"][k], u_pred=g[f"{tag}_u_pred"][k])
        tw.assert_margins(p, info)
        out = device_post(p, s, int(g[f"{tag}_step"][k]), counter_on_device=bool(k % 2))
        want = {n: g[f"{tag}_{n}"][k] for n in ("predator_pos", "root_states", "obs", "rew", "reset_buf", "curr_episode_step", "episode_length_buf", "episode_sums")}
        check_call(p, s, out, info, want, extra_ulp=2)
        np.testing.assert_array_equal(out["obs"][:, 15] != 0, g[f"{tag}_sense_flag"][k] != 0)
        state = dict(state, **{n: out[n] for n in ("predator_pos", "obs", "curr_episode_step", "episode_length_buf", "episode_sums")})


@pytest.mark.parametrize("custom", [0, 1])
def test_kernel_reproduces_the_recorded_root_reset(golden_dir, custom):
    """game_reset.npz: every listed env is made done through ``ll_reset``; root state and predator placement bit-equal to the reference's."""
    g = load(golden_dir, "game_reset.npz")
    t = f"c{custom}"
    p = json.loads(str(g[f"{t}_params"]))
    n, ids = g[f"{t}_env_origins"].shape[0], g[f"{t}_env_ids"]
    ll_reset = np.zeros(n, bool); ll_reset[ids] = True
    root_in = g[f"{t}_in_root_states"].copy()
    root_in[:, 3:7] = [0, 0, 0, 1]
    pred_in = (root_in[:, :3] + np.array([3.0, 0.5, 0.0], F)).astype(F)             # 3 m ahead: nobody is captured
    s = dict(command=np.zeros((n, 6), F), root_states=root_in, env_origins=g[f"{t}_env_origins"], ll_rew=np.zeros(n, F), ll_reset=ll_reset, predator_pos=pred_in,
             obs=np.zeros((n, 19), F), curr_episode_step=np.full(n, 5, np.int64), episode_length_buf=np.full(n, 9, np.int64), episode_sums=np.zeros((2, n), F))
    out = device_post(p, s, int(g[f"{t}_step"]))
    np.testing.assert_array_equal(out["reset_buf"], ll_reset)
    np.testing.assert_array_equal(out["root_states"][ids].view(np.uint32), g[f"{t}_root_states"][ids].view(np.uint32))
    np.testing.assert_array_equal(out["predator_pos"][ids].view(np.uint32), g[f"{t}_predator_pos"][ids].view(np.uint32))
    rest = np.setdiff1d(np.arange(n), ids)
    np.testing.assert_array_equal(out["root_states"][rest], root_in[rest]); np.testing.assert_array_equal(out["predator_pos"][rest], pred_in[rest])
    assert (out["curr_episode_step"][ids] == 0).all() and (out["curr_episode_step"][rest] == 6).all()
    assert (out["episode_length_buf"][ids] == 0).all() and (out["episode_length_buf"][rest] == 9).all()


@pytest.mark.parametrize("n,radius", [(1, -1.0), (63, 6.0), (4096, -1.0), (4097, 5.0)])
def test_kernels_match_the_twin_on_ragged_sizes(n, radius):
    """Seeded state through the twin at sizes with a ragged last workgroup (the kernels run 256 threads per workgroup)."""
    p = tw.params(num_envs=n, seed=1234 + n, env_radius=radius, custom_origins=n % 2)
    step = 40 + n
    s = synthetic_state(p, n, seed=n, step=step)
    raw = np.random.default_rng(n).uniform(-4, 4, (n, 6)).astype(F)
    c_dev, ll_dev = device_pre(p, raw)
    c_tw, ll_tw = tw.pre(p, raw)
    np.testing.assert_array_equal(c_dev.view(np.uint32), c_tw.view(np.uint32)); np.testing.assert_array_equal(ll_dev.view(np.uint32), ll_tw.view(np.uint32))
    want, info = tw.post(p, s, step=step)
    tw.assert_margins(p, info)
    out = device_post(p, s, step, counter_on_device=True)
    check_call(p, s, out, info, want, extra_ulp=2)
    if n >= 63:
        assert want["reset_buf"].any() and not want["reset_buf"].all() and info["visible"].any() and not info["visible"].all()


# ----------------------------------------------------------------------------- env helpers
def write_ll_checkpoint(path, seed=0, zero_actions=False):
    """A low-level a1 checkpoint in the runner's format: seeded random-init actor (or one whose actions are exactly zero: the robot stands)."""
    from legged_games_gym_amd.envs import task_registry
    from legged_games_gym_amd.rl import ActorCritic
    from legged_games_gym_amd.utils.helpers import class_to_dict
    env_cfg, train_cfg = task_registry.get_cfgs("a1")
    torch.manual_seed(seed)
    ac = ActorCritic(env_cfg.env.num_observations, env_cfg.env.num_observations, env_cfg.env.num_actions, **class_to_dict(train_cfg.policy))
    if zero_actions:
        with torch.no_grad():
            ac.actor[-1].weight.zero_(); ac.actor[-1].bias.zero_()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save({"model_state_dict": ac.state_dict(), "optimizer_state_dict": {}, "iter": 0, "infos": None}, path)
    return path


def make_game(ckpt, n=512, seed=1, mesh="plane", radius=None, noise=True):
    from legged_games_gym_amd.envs.a1_game import HighLevelGame, HighLevelGameFlatCfg
    from legged_games_gym_amd.utils import get_args, set_seed
    from legged_games_gym_amd.utils.helpers import class_to_dict, parse_sim_params
    cfg = HighLevelGameFlatCfg()
    cfg.env.num_envs, cfg.env.ll_policy_path, cfg.env.env_radius = n, ckpt, radius
    cfg.terrain.mesh_type, cfg.noise.add_noise, cfg.seed = mesh, noise, seed
    args = get_args(["--headless", "--sim_device", DEV, "--rl_device", DEV])
    set_seed(seed)
    return HighLevelGame(cfg, parse_sim_params(args, {"sim": class_to_dict(cfg.sim)}), args.physics_engine, DEV, True)


def snapshot(env, command):
    """The inputs of ``lg_game_post`` as the twin takes them."""
    ll = env.ll_env
    c = lambda x: x.detach().cpu().numpy().copy()
    return dict(command=c(command), root_states=c(ll.root_states), env_origins=c(ll.env_origins), ll_rew=c(ll.rew_buf), ll_reset=c(ll.reset_buf),
                predator_pos=c(env.predator_pos), obs=c(env.obs_buf), curr_episode_step=c(env.curr_episode_step), episode_length_buf=c(env.episode_length_buf),
                episode_sums=c(env._episode_sums))


def outputs(env):
    c = lambda x: x.detach().cpu().numpy().copy()
    return dict(root_states=c(env.ll_env.root_states), predator_pos=c(env.predator_pos), obs=c(env.obs_buf), rew=c(env.rew_buf), reset_buf=c(env.reset_buf),
                curr_episode_step=c(env.curr_episode_step), episode_length_buf=c(env.episode_length_buf), episode_sums=c(env._episode_sums))


def yaw_of(root):
    z, w = root[:, 5], root[:, 6]
    return 2.0 * torch.atan2(z, w)


def place_ahead(env, ids, dist, behind=False):
    """Write ``predator_pos`` of ``ids`` to ``dist`` metres straight ahead of (or behind) the prey, through the public attributes."""
    root = env.ll_env.root_states[ids]
    yaw = yaw_of(root) + (math.pi if behind else 0.0)
    d = torch.as_tensor(dist, device=root.device, dtype=torch.float32)
    env.predator_pos[ids, 0] = root[:, 0] + d * torch.cos(yaw)
    env.predator_pos[ids, 1] = root[:, 1] + d * torch.sin(yaw)


def settle(env, park=4.0, quiet=40, limit=300):
    """Zero command, predators parked ``park`` metres behind: step until no env has been reset for ``quiet`` consecutive steps (the standing robots
    have come to rest; one that fell on its first landing has been reset by the low-level env and has settled too)."""
    env.reset()
    env.ll_env.root_states[:, 7:13] = 0
    zero = torch.zeros(env.num_envs, env.num_actions, device=DEV)
    everyone = torch.arange(env.num_envs, device=DEV)
    calm = 0
    for _ in range(limit):
        place_ahead(env, everyone, park, behind=True)
        env.step(zero.clone())
        calm = 0 if bool(env.reset_buf.any()) else calm + 1
        if calm >= quiet:
            return
    raise AssertionError("the standing robots did not come to rest")


# ----------------------------------------------------------------------------- env step = its parts
GUARD = 0.15          # rad: predators whose bearing comes this close to the edge of the field of view are put back straight ahead


def test_env_step_equals_its_parts_and_the_twin(tmp_path):
    """Two identically seeded envs: A calls ``step``; on B the test calls pre -> act_inference -> ll_env.step -> post by hand and checks post against
    the twin from a snapshot of its inputs.  A and B must agree bit for bit at every step.  The test arranges captures (32 predators start 1.2 m
    ahead of their prey and home in at 2 m/s: 0.04 m per step, 18 steps to the capture distance) and low-level time-outs (32 other envs are 5
    steps from the low-level episode end).  Bearings are kept away from the edge of the field of view by re-placing, on both envs alike, any predator
    that comes within GUARD of it (a bearing moves by less than that per step), so the twin comparison of the flags needs no exclusion.  What is
    left to the trajectory (a predator re-placed by a reset, the step at which a chaser crosses the capture distance) is fixed by the seeds: the kernels
    and the low-level step are deterministic, and the section-3 margins are asserted on the twin's values at every step before anything is compared."""
    from legged_games_gym_amd import capi
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    N = 512
    A, B = make_game(ckpt, N, seed=7), make_game(ckpt, N, seed=7)
    for env in (A, B):
        torch.manual_seed(70)             # reset_idx from the host draws from torch's generator
        env.reset()
    assert torch.equal(A.ll_env.root_states, B.ll_env.root_states) and torch.equal(A.predator_pos, B.predator_pos) and torch.equal(A.obs_buf, B.obs_buf)
    chase, timed = torch.arange(0, 32, device=DEV), torch.arange(32, 64, device=DEV)
    for env in (A, B):
        place_ahead(env, chase, 1.2)
        env.ll_env.episode_length_buf[timed] = int(env.ll_env.max_episode_length) - 5
    p = unpack_params(B._P)
    gen = torch.Generator().manual_seed(5)
    captured, ll_alone, clipped = 0, 0, 0
    stream = torch.cuda.current_stream().cuda_stream
    for k in range(30):
        # keep every bearing clear of the field-of-view edge (public attributes, both envs alike)
        s0 = snapshot(A, torch.zeros(N, 6))
        _, _, angle, _, _ = tw.sense(p, s0["predator_pos"], s0["root_states"][:, :3], s0["root_states"][:, 3:7], s0["obs"][:, 9:12])
        near = torch.from_numpy(np.nonzero(np.abs(np.abs(angle) - F(p["half_fov"])) < GUARD)[0]).to(DEV)
        if len(near):
            for env in (A, B):
                rel = env.predator_pos[near, :2] - env.ll_env.root_states[near, :2]
                place_ahead(env, near, rel.norm(dim=1))
        cmd = (3.0 * torch.randn(N, 6, generator=gen)).to(DEV)               # well outside the ranges: the clip is exercised
        to_prey = A.ll_env.root_states[chase, :2] - A.predator_pos[chase, :2]
        cmd[chase, 4:6] = 2.0 * to_prey / to_prey.norm(dim=1, keepdim=True)
        cmd[64:, 4:6] *= 0.1                                                 # the other predators drift slowly
        clipped += int((cmd[:, [0, 1, 4, 5]].abs() > 2.0).sum())
        ca, cb = cmd.clone(), cmd.clone()
        A.step(ca)
        # B, by hand
        ll = B.ll_env
        bufs = B._bind_command(cb, B.obs_buf)
        capi.game_pre(B._P, bufs, stream)
        actions = B.ll_policy(ll.obs_buf)
        ll.step(actions)
        torch.cuda.synchronize()
        s = snapshot(B, cb)
        capi.game_post(B._P, bufs, ll.common_step_counter, stream)
        torch.cuda.synchronize()
        want, info = tw.post(p, s, step=ll.common_step_counter)
        tw.assert_margins(p, info)
        check_call(p, s, outputs(B), info, want, extra_ulp=2)
        assert torch.equal(ca, cb)
        for name in ("obs_buf", "rew_buf", "reset_buf", "predator_pos", "curr_episode_step"):
            assert torch.equal(getattr(A, name), getattr(B, name)), (k, name)
        assert torch.equal(A.ll_env.root_states, B.ll_env.root_states) and torch.equal(A.ll_env.commands, B.ll_env.commands), k
        captured += int(info["capture"].sum())
        ll_alone += int(((s["ll_reset"] != 0) & ~info["capture"] & ~info["radius"]).sum())
    assert captured >= 8 and ll_alone >= 8 and clipped > 0, (captured, ll_alone, clipped)


# ----------------------------------------------------------------------------- known answers
def test_pursuit_time_reset_placement_and_occlusion(tmp_path):
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), zero_actions=True)
    N = 64
    env = make_game(ckpt, N, seed=2, noise=False)
    assert (env.num_envs, env.num_obs, env.num_actions, env.num_privileged_obs) == (N, 19, 6, None) and not hasattr(env, "_sim")
    assert env.max_episode_length == 1000 and env.extras == {} and env.get_privileged_observations() is None
    settle(env)
    everyone = torch.arange(N, device=DEV)
    # occlusion: a predator straight ahead is seen; moved straight behind it is not, and the previous sensed position is repeated
    zero = torch.zeros(N, 6, device=DEV)
    place_ahead(env, everyone, 2.0)
    obs, _, _, dones, _ = env.step(zero.clone())
    assert not bool(dones.any()) and bool((obs[:, 15] == 1).all())
    seen = obs[:, 9:12].clone()
    assert torch.equal(seen, env.predator_pos - env.ll_env.root_states[:, :3])
    place_ahead(env, everyone, 2.0, behind=True)
    obs, _, _, dones, _ = env.step(zero.clone())
    assert bool((obs[:, 15] == 0).all()) and bool((obs[:, 14] == 1).all()) and torch.equal(obs[:, 9:12], seen) and torch.equal(obs[:, 6:9], seen)
    assert torch.equal(obs[:, 16:19], env.ll_env.root_states[:, :3] - env.predator_pos)
    assert env.get_observations() is env.obs_buf

    # pursuit: prey commanded to stand, predator at (d0, 0) commanded (-v, 0)
    d0, v = 2.0, 2.0
    dt = env.ll_env.cfg.control.decimation * env.ll_env.cfg.sim.dt
    expect = math.ceil((d0 - env.capture_dist) / (v * dt))
    assert expect == 38
    env.predator_pos[:, 0] = env.ll_env.root_states[:, 0] + d0
    env.predator_pos[:, 1] = env.ll_env.root_states[:, 1]
    cmd = torch.zeros(N, 6, device=DEV); cmd[:, 4] = -v
    first = torch.zeros(N, dtype=torch.long, device=DEV)
    steps_before = env.curr_episode_step.clone()
    for k in range(1, expect + 2):
        obs, _, rew, dones, _ = env.step(cmd.clone())
        fresh = dones & (first == 0)
        first[fresh] = k
        if k < expect - 1:
            assert not bool(dones.any()), k                                       # not before
        if bool(fresh.any()):
            # after a reset: shifted 100-fill, offsets of 1..10 m with one common sign, predator z = 0.3, episode step 0
            ids = fresh.nonzero().flatten()
            assert bool((obs[ids, 0:9] == 100).all()) and bool((obs[ids, 12:15] == 0).all())
            off = env.ll_env.root_states[ids, :2] - env.predator_pos[ids, :2]
            assert bool(((off.abs() >= 1.0 - 1e-5) & (off.abs() <= 10.0 + 1e-5)).all()) and bool((off[:, 0].sign() == off[:, 1].sign()).all())
            assert bool((env.predator_pos[ids, 2] == 0.3).all()) and bool((env.curr_episode_step[ids] == 0).all())
            assert torch.equal(obs[ids, 16:19], env.ll_env.root_states[ids, :3] - env.predator_pos[ids])
            vis = obs[ids, 15] == 1
            assert torch.equal(obs[ids][vis][:, 9:12], -obs[ids][vis][:, 16:19]) and bool((obs[ids][~vis][:, 9:12] == 100).all())
        alive = first == 0
        assert torch.equal(env.curr_episode_step[alive], steps_before[alive] + k)
        cmd[~alive, 4] = 0.0                                                     # a re-placed predator stays where it is
    assert bool(((first >= expect - 1) & (first <= expect + 1)).all()), first.tolist()
    assert torch.isfinite(rew).all() and bool((rew >= 0).all())


def test_radius_ends_the_episode_when_the_predator_leaves(tmp_path):
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), zero_actions=True)
    N, R = 64, 3.0
    env = make_game(ckpt, N, seed=4, radius=R, noise=False)
    settle(env, park=2.0)                                                        # (inside the radius, outside the capture distance)
    org = env.ll_env.env_origins
    env.predator_pos[:, 0] = org[:, 0] + 1.5
    env.predator_pos[:, 1] = org[:, 1]
    cmd = torch.zeros(N, 6, device=DEV); cmd[:, 4] = 2.0
    expect = 38                                                                  # 1.5 + 0.04 k > 3.0 first at k = 38 (37 steps: 2.98 m)
    for k in range(1, expect + 1):
        _, _, _, dones, _ = env.step(cmd.clone())
        prey_r = (env.ll_env.root_states[:, :2] - org[:, :2]).norm(dim=1)
        if k < expect:
            assert not bool(dones.any()), k
            assert bool((prey_r < 1.0).all())
    assert bool(dones.all())


# ----------------------------------------------------------------------------- graph
def test_graphed_step_equals_eager_steps(tmp_path):
    """``make_graphed_step`` (3 warm-up steps, then 20 replays of the five captured launches) equals 23 eager ``step`` calls from the same state."""
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    N = 512
    A, B = make_game(ckpt, N, seed=9), make_game(ckpt, N, seed=9)
    torch.manual_seed(11)
    net = torch.nn.Sequential(torch.nn.Linear(19, 64), torch.nn.ELU(), torch.nn.Linear(64, 6)).to(DEV)

    def policy(obs):
        with torch.no_grad():
            return 2.0 * torch.tanh(net(obs * 0.05))
    timed = torch.arange(0, 32, device=DEV)
    for env in (A, B):
        torch.manual_seed(90)             # reset_idx from the host draws from torch's generator
        env.reset()
        place_ahead(env, torch.arange(32, 64, device=DEV), 0.8)
        env.ll_env.episode_length_buf[timed] = int(env.ll_env.max_episode_length) - 12
    replay = A.make_graphed_step(policy, warmup=3)
    for _ in range(3):
        B.step(policy(B.obs_buf))
    assert A.ll_env.common_step_counter == B.ll_env.common_step_counter
    resets = 0
    for k in range(20):
        oa, _, ra, da, _ = replay()
        ob, _, rb, db, _ = B.step(policy(B.obs_buf))
        torch.cuda.synchronize()
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db), k
        assert torch.equal(A.predator_pos, B.predator_pos) and torch.equal(A.ll_env.root_states, B.ll_env.root_states), k
        assert torch.equal(A.curr_episode_step, B.curr_episode_step) and torch.equal(A.ll_env.obs_buf, B.ll_env.obs_buf), k
        resets += int(da.sum())
    assert resets >= 32 and A.ll_env.common_step_counter == B.ll_env.common_step_counter


# ----------------------------------------------------------------------------- surface
def test_registry_runner_and_play_surface(tmp_path, monkeypatch, game_registered):
    import legged_games_gym_amd.utils.task_registry as tr_mod
    from legged_games_gym_amd.scripts.play import play
    from legged_games_gym_amd.utils import get_args
    from legged_games_gym_amd.utils.helpers import class_to_dict, get_load_path
    reg = game_registered
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    monkeypatch.setattr(tr_mod, "LEGGED_GYM_ROOT_DIR", str(tmp_path))
    env_cfg, train_cfg = reg.get_cfgs("high_level_game")
    env_cfg.terrain.mesh_type, env_cfg.env.ll_policy_path = "plane", ckpt
    args = get_args(["--task", "high_level_game", "--num_envs", "64", "--headless", "--sim_device", DEV, "--rl_device", DEV, "--max_iterations", "2"])
    a1_before = json.dumps(class_to_dict(reg.get_cfgs("a1")[0]), default=str)
    env, _ = reg.make_env("high_level_game", args)
    assert (env.num_envs, env.num_obs, env.num_actions) == (64, 19, 6) and not env.ll_env.custom_origins
    assert json.dumps(class_to_dict(reg.get_cfgs("a1")[0]), default=str) == a1_before                  # the registered a1 cfg is not mutated
    assert reg.get_cfgs("a1")[0].rewards.scales.torques == -0.0002
    assert env.ll_env.cfg.rewards.scales.torques == -5.0 and env.ll_env.cfg.terrain.mesh_type == "plane"
    runner, cfg = reg.make_alg_runner(env, "high_level_game", args)
    assert runner._fused is None                                                 # the generic VecEnv path
    runner.learn(num_learning_iterations=2, init_at_random_ep_len=True)
    obs = env.get_observations()
    assert obs.shape == (64, 19) and torch.isfinite(obs).all() and torch.isfinite(env.rew_buf).all()
    acts = runner.get_inference_policy(device=env.device)(obs)
    assert acts.shape == (64, 6) and torch.isfinite(acts).all()
    path = get_load_path(str(tmp_path / "logs" / "high_level_game_flat"))
    assert path.endswith("model_2.pt")
    env2 = play(get_args(["--task", "high_level_game", "--headless", "--sim_device", DEV, "--rl_device", DEV]), steps=5)
    assert env2.num_envs == 50 and torch.isfinite(env2.obs_buf).all() and not env2.ll_env.cfg.noise.add_noise


def test_registered_trimesh_terrain_runs(tmp_path):
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    env = make_game(ckpt, 64, seed=1, mesh="trimesh")
    assert env.ll_env.custom_origins and env._P.custom_origins == 1 and env.cfg.terrain.curriculum
    obs, _ = env.reset()
    for _ in range(10):
        obs, _, rew, dones, _ = env.step(torch.randn(64, 6, device=DEV))
    assert obs.shape == (64, 19) and torch.isfinite(obs).all() and torch.isfinite(rew).all() and torch.isfinite(env.predator_pos).all()


def test_missing_low_level_checkpoint_says_to_train_a1(tmp_path, monkeypatch):
    import legged_games_gym_amd.envs.a1_game.high_level_game as mod
    monkeypatch.setattr(mod, "LEGGED_GYM_ROOT_DIR", str(tmp_path))
    with pytest.raises(RuntimeError, match="Train the a1 task first"):
        make_game(None, 16)
