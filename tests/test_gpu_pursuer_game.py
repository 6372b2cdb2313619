"""-m gpu: the scripted pursuer -- ``lg_pursuer_post`` against the float32 speed limit on every episode step, against the reference's
recorded step (tests/golden/pursuer_step.npz) and the NumPy twin, the ignored command columns, a known answer (pursuit at the shrinking
speed limit, capture time), and every step path of ``ScriptedPredatorGame`` against its parts.  Nothing here reads the reference tree."""
import json
import math

import numpy as np
import pytest
import torch

from tests import game_twin as tw
from tests import pursuer_twin as pt
from tests.game_fixtures import LOCOMOTION_TASKS, check_call, load
from tests.pursuer_fixtures import WANT, call_inputs, initial_state, synthetic_state
from tests.test_gpu_game import device_post, device_pre, outputs, pack_params, settle, snapshot, unpack_params, write_ll_checkpoint
from tests.test_gpu_game_policy import high_level_actor

pytestmark = pytest.mark.gpu
F = np.float32
DEV = "cuda:0"
STATE = ("root_states", "predator_pos", "obs", "rew", "reset_buf", "curr_episode_step", "episode_length_buf", "episode_sums")


# ----------------------------------------------------------------------------- the kernel without an env
def pack_pursuer(q):
    from legged_games_gym_amd import capi
    Q = capi.lg_pursuer_params()
    Q.max_lin_vel, Q.min_lin_vel, Q.gain, Q.max_episode_length = float(q["max_lin_vel"]), float(q["min_lin_vel"]), float(q["gain"]), int(q["max_episode_length"])
    return Q


def device_pursuer_post(p, q, s, step, counter_on_device=False, want_command=True):
    """``lg_pursuer_post`` on the arrays of a twin state dict, uploaded as they are -> the dict layout of ``pursuer_twin.post`` plus ``predator_command``
    (NaN-filled before the launch; None when the kernel is given a null pointer)."""
    from legged_games_gym_amd import capi
    n = s["root_states"].shape[0]
    t = {k: torch.from_numpy(np.ascontiguousarray(s[k])).to(DEV) for k in ("command", "root_states", "env_origins", "ll_rew", "predator_pos", "obs", "curr_episode_step",
                                                                           "episode_length_buf", "episode_sums")}
    t["ll_reset"] = torch.from_numpy(np.ascontiguousarray(s["ll_reset"]).astype(bool)).to(DEV)
    t["rew"], t["reset_buf"] = torch.full((n,), -3.0, device=DEV), torch.zeros(n, dtype=torch.bool, device=DEV)
    t["counter"] = torch.tensor([step], dtype=torch.int64, device=DEV)
    t["predator_command"] = torch.full((n, 2), float("nan"), device=DEV)
    for k in ("command", "root_states", "env_origins", "ll_rew", "predator_pos", "obs", "episode_sums"):
        assert t[k].dtype == torch.float32
    assert t["curr_episode_step"].dtype == torch.int64 and t["obs"].shape == (n, 19) and t["root_states"].shape == (n, 13) and t["episode_sums"].shape == (2, n)
    B = capi.game_buffers({"command": t["command"].data_ptr(), "ll_root_states": t["root_states"].data_ptr(), "ll_env_origins": t["env_origins"].data_ptr(),
                           "ll_rew_buf": t["ll_rew"].data_ptr(), "ll_reset_buf": t["ll_reset"].data_ptr(), "ll_step_counter": t["counter"].data_ptr(),
                           "predator_pos": t["predator_pos"].data_ptr(), "obs": t["obs"].data_ptr(), "rew": t["rew"].data_ptr(), "reset_buf": t["reset_buf"].data_ptr(),
                           "curr_episode_step": t["curr_episode_step"].data_ptr(), "episode_length_buf": t["episode_length_buf"].data_ptr(),
                           "episode_sums": t["episode_sums"].data_ptr()})
    capi.pursuer_post(pack_params(dict(p, num_envs=n)), pack_pursuer(q), B, t["predator_command"].data_ptr() if want_command else None,
                      -1 if counter_on_device else step, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = {k: t[k].cpu().numpy() for k in STATE}
    out["predator_command"] = t["predator_command"].cpu().numpy() if want_command else None
    assert int(t["counter"][0]) == step and np.array_equal(t["command"].cpu().numpy(), s["command"])          # inputs are left alone
    if not want_command:
        assert bool(torch.isnan(t["predator_command"]).all())
    return out


@pytest.mark.parametrize("L", [1000, 997])
def test_speed_limit_is_bit_exact_on_every_episode_step(L):
    """One launch, 2 L + 1 envs, ``ep`` = 0 .. 2 L, the prey 50 m away on both axes: every velocity is saturated, i.e. a copy of ``lim`` (of
    +lim while it is positive, of lim itself once it is negative), and must equal the float32 restatement bit for bit -- the library's
    plain division is not correctly rounded; the kernel's quotient is.  L = 1000 is the registered task's."""
    n = 2 * L + 1
    p, q = tw.params(num_envs=n), pt.pursuer_params(max_episode_length=L)
    root = np.zeros((n, 13), F)
    root[:, :3], root[:, 6] = (50.0, 50.0, 0.3), 1.0
    s = dict(command=np.zeros((n, 6), F), root_states=root, env_origins=np.zeros((n, 3), F), ll_rew=np.zeros(n, F), ll_reset=np.zeros(n, bool),
             predator_pos=np.tile(np.array([0.0, 0.0, 0.3], F), (n, 1)), obs=np.zeros((n, 19), F), curr_episode_step=np.arange(-1, 2 * L, dtype=np.int64),
             episode_length_buf=np.ones(n, np.int64), episode_sums=np.zeros((2, n), F))
    out = device_pursuer_post(p, q, s, step=5)
    ep = np.arange(0, 2 * L + 1)
    lim = pt.speed_limit(q, ep)
    assert lim[0] == F(2.0) and lim[L] == F(0.01) and (lim[: L + 1] > 0).all() and (lim[L + int(0.006 * L) + 1:] < 0).all()
    got = out["predator_command"]
    bad = np.nonzero((got.view(np.uint32) != lim.view(np.uint32)[:, None]).any(axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} of {n} limits differ, first at ep {ep[bad[:5]].tolist()}: {got[bad[:5], 0].tolist()} vs {lim[bad[:5]].tolist()}"
    assert not out["reset_buf"].any() and np.array_equal(out["curr_episode_step"], ep)
    want, _ = pt.post(p, q, s, step=5)
    np.testing.assert_array_equal(out["predator_pos"].view(np.uint32), want["predator_pos"].view(np.uint32))


@pytest.mark.parametrize("tag", ["a", "b"])
def test_kernel_reproduces_the_recorded_reference_step(golden_dir, tag):
    """pursuer_step.npz through the DEVICE, the state carried by the device's own outputs (the episode sums by the fixture's: see
    tests/pursuer_fixtures.py); the bounds tests/test_gpu_game.py uses for ``lg_game_post``: bit-equal, the reward and the sums behind the
    device's 1-ulp sqrt 2 ulp wider than on the CPU.  The step counter is passed by value on even calls and read from the device on odd ones."""
    g = load(golden_dir, "pursuer_step.npz")
    p, q = json.loads(str(g[f"{tag}_params"])), json.loads(str(g[f"{tag}_pursuer_params"]))
    state = initial_state(g, tag)
    for k in range(g[f"{tag}_step"].shape[0]):
        s = call_inputs(g, tag, k, p, state)
        command, _ = device_pre(p, g[f"{tag}_in_command"][k])
        np.testing.assert_array_equal(command.view(np.uint32), s["command"].view(np.uint32))
        want = {n: g[f"{tag}_{n}"][k] for n in WANT}
        _, info = pt.post(p, q, s, u_root=g[f"{tag}_u_root"][k], u_pred=g[f"{tag}_u_pred"][k])
        tw.assert_margins(p, info)
        out = device_pursuer_post(p, q, s, int(g[f"{tag}_step"][k]), counter_on_device=bool(k % 2))
        np.testing.assert_array_equal(out["predator_command"].view(np.uint32), want["predator_command"].view(np.uint32))
        check_call(p, s, out, info, want, extra_ulp=2)
        np.testing.assert_array_equal(out["obs"][:, 15] != 0, want["sense_flag"] != 0)
        alive = ~want["reset_buf"].astype(bool)
        np.testing.assert_array_equal(out["predator_pos"][alive].view(np.uint32), want["predator_integrated"][alive].view(np.uint32))       # before the resets
        state = dict(state, **{n: out[n] for n in ("predator_pos", "obs", "curr_episode_step", "episode_length_buf")})
        state["episode_sums"] = want["episode_sums"]


@pytest.mark.parametrize("radius", [-1.0, 5.0])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_kernel_matches_the_twin_on_ragged_sizes(n, radius):
    """Seeded state through the twin at one thread and at a workgroup edge on either side (256 threads per workgroup), radius off and on."""
    p, q = tw.params(num_envs=n, seed=4321 + n, env_radius=radius, custom_origins=n % 2), pt.pursuer_params()
    step = 70 + n
    s = synthetic_state(p, q, n, seed=n + (1000 if radius >= 0 else 0), step=step)
    want, info = pt.post(p, q, s, step=step)
    tw.assert_margins(p, info)
    out = device_pursuer_post(p, q, s, step, counter_on_device=True)
    np.testing.assert_array_equal(out["predator_command"].view(np.uint32), info["predator_command"].view(np.uint32))
    check_call(p, s, out, info, want, extra_ulp=2)
    if n >= 255:
        assert want["reset_buf"].any() and not want["reset_buf"].all() and info["visible"].any() and not info["visible"].all()
        unsat, sat, neg = pt.branch_shares(info)
        assert min(unsat, sat, neg) > 0, (unsat, sat, neg)


def test_command_columns_are_ignored_and_the_velocity_output_is_optional():
    n = 300
    p, q = tw.params(num_envs=n, seed=77), pt.pursuer_params()
    s = synthetic_state(p, q, n, seed=5, step=9)
    huge, zero = dict(s, command=s["command"].copy()), dict(s, command=s["command"].copy())
    huge["command"][:, 4], huge["command"][:, 5], zero["command"][:, 4:6] = 1e6, -1e6, 0.0
    a, b = device_pursuer_post(p, q, huge, 9), device_pursuer_post(p, q, zero, 9)
    for k in STATE + ("predator_command",):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    # lg_game_post on the same inputs integrates columns 4:6 and lands elsewhere
    g = device_post(p, s, 9)
    alive = ~(a["reset_buf"] | g["reset_buf"])
    assert alive.sum() > n // 2 and (np.abs(s["command"][alive, 4:6]) > 0.1).all(axis=1).any()
    assert not np.array_equal(g["predator_pos"][alive], a["predator_pos"][alive])
    # a null predator_command: the launch runs and everything else is unchanged
    c = device_pursuer_post(p, q, s, 9, want_command=False)
    d = device_pursuer_post(p, q, s, 9)
    for k in STATE:
        np.testing.assert_array_equal(c[k], d[k], err_msg=k)
    np.testing.assert_array_equal(d["predator_command"], a["predator_command"])


# ----------------------------------------------------------------------------- env helpers
def make_scripted(ckpt, n=64, seed=1, radius=None, noise=True):
    from legged_games_gym_amd.envs.a1_game import ScriptedPredatorGame, ScriptedPredatorGameCfg
    from legged_games_gym_amd.utils import get_args, set_seed
    from legged_games_gym_amd.utils.helpers import class_to_dict, parse_sim_params
    cfg = ScriptedPredatorGameCfg()
    cfg.env.num_envs, cfg.env.ll_policy_path, cfg.env.env_radius = n, ckpt, radius
    cfg.terrain.mesh_type, cfg.noise.add_noise, cfg.seed = "plane", noise, seed
    args = get_args(["--headless", "--sim_device", DEV, "--rl_device", DEV])
    set_seed(seed)
    return ScriptedPredatorGame(cfg, parse_sim_params(args, {"sim": class_to_dict(cfg.sim)}), args.physics_engine, DEV, True)


def unpack_pursuer(Q):
    return dict(max_lin_vel=float(Q.max_lin_vel), min_lin_vel=float(Q.min_lin_vel), gain=float(Q.gain), max_episode_length=int(Q.max_episode_length))


def two_scripted(tmp_path, seed, reset_seed, n=64):
    """Two identically seeded envs with spread episode steps (a few past max_episode_length: the negative limit) and 8 low-level time-outs ahead."""
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    A, B = make_scripted(ckpt, n, seed=seed), make_scripted(ckpt, n, seed=seed)
    for env in (A, B):
        torch.manual_seed(reset_seed)             # reset_idx from the host draws from torch's generator
        env.reset()
        env.curr_episode_step[:] = torch.arange(n, device=DEV) * (1300 // n)
        env.ll_env.episode_length_buf[:8] = int(env.ll_env.max_episode_length) - 6
    assert torch.equal(A.ll_env.root_states, B.ll_env.root_states) and torch.equal(A.predator_pos, B.predator_pos) and torch.equal(A.obs_buf, B.obs_buf)
    return A, B


def assert_same_state(A, B, k):
    for name in ("obs_buf", "rew_buf", "reset_buf", "predator_pos", "predator_command", "curr_episode_step"):
        assert torch.equal(getattr(A, name), getattr(B, name)), (k, name)
    assert torch.equal(A.ll_env.root_states, B.ll_env.root_states) and torch.equal(A.ll_env.obs_buf, B.ll_env.obs_buf), k
    assert torch.equal(A.ll_env.commands, B.ll_env.commands), k


def assert_within_limit(env, ep_before, k):
    """|predator_command| <= |lim| of the env's episode step (lim > 0: the clamp; lim < 0: the command IS lim)."""
    lim = pt.speed_limit(unpack_pursuer(env._Q), ep_before.cpu().numpy() + 1)
    v = env.predator_command.cpu().numpy()
    assert (np.abs(v) <= np.abs(lim)[:, None]).all(), k
    assert (v[lim < 0] == lim[lim < 0, None]).all(), k


# ----------------------------------------------------------------------------- 5. known answer
def test_pursuit_at_the_shrinking_speed_limit_and_capture_time(tmp_path):
    """Standing prey (zero-action low-level policy, zero command), the predator 3 m from it along x.  While 2 |dx| exceeds the limit the predator
    moves dt * lim_k per step along x: after 20 steps its displacement is the float64 sum of dt * lim_k to 1e-4 m (80 float32 additions at
    coordinates below 32 m: at most 80 half-ulps of 1.9e-6 m).  The capture step follows from the same law iterated in float64 with the prey
    where it stood: saturated approach, then dx shrinking by 1 - gain * dt per step, until |d| < capture_dist; +-1 step for the prey's sway."""
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), zero_actions=True)
    N = 64
    env = make_scripted(ckpt, N, seed=2, noise=False)
    assert (env.num_envs, env.num_obs, env.num_actions) == (N, 19, 6) and env.max_episode_length == 1000 and env._Q.max_episode_length == 1000
    assert env.predator_command.shape == (N, 2) and env.TASK == "scripted_predator_game"
    settle(env)
    q = unpack_pursuer(env._Q)
    dt = env.ll_env.cfg.control.decimation * env.ll_env.cfg.sim.dt
    ep0 = np.where(np.arange(N) < N // 2, 0, 400).astype(np.int64)
    env.curr_episode_step[:] = torch.from_numpy(ep0).to(DEV)
    env.predator_pos[:, 0] = env.ll_env.root_states[:, 0] + 3.0
    env.predator_pos[:, 1] = env.ll_env.root_states[:, 1]
    start = env.predator_pos.clone()
    rel0 = (env.ll_env.root_states[:, :2] - env.predator_pos[:, :2]).double().cpu().numpy()
    # the law in float64 with the prey parked
    expect = np.zeros(N, np.int64)
    for e in range(N):
        d, k = rel0[e].copy(), 0
        while np.hypot(*d) >= env.capture_dist:
            k += 1
            lim = float(pt.speed_limit(q, np.array([ep0[e] + k]))[0])
            d -= dt * np.clip(q["gain"] * d, -lim, lim)
        expect[e] = k
    assert 40 < expect.min() and expect.max() < 160 and expect[0] != expect[-1], expect
    cmd = torch.zeros(N, 6, device=DEV)
    cmd[:, 4:6] = 2.0                                                               # ignored: would carry the predator AWAY from the prey
    first = torch.zeros(N, dtype=torch.long, device=DEV)
    for k in range(1, int(expect.max()) + 3):
        before = env.curr_episode_step.clone()
        obs, _, rew, dones, _ = env.step(cmd.clone())
        fresh = dones & (first == 0)
        first[fresh] = k
        alive = first == 0
        if k <= 20:
            assert not bool(dones.any()), k
            assert_within_limit(env, before, k)
            lim_k = pt.speed_limit(q, ep0 + k)
            assert torch.equal(env.predator_command[:, 0], torch.from_numpy(-lim_k).to(DEV)), k        # saturated along x, towards the prey
        if k == 20:
            moved = (env.predator_pos - start).double().cpu().numpy()
            want = -np.array([sum(dt * float(pt.speed_limit(q, np.array([e0 + j]))[0]) for j in range(1, 21)) for e0 in ep0])
            assert np.abs(moved[:, 0] - want).max() <= 1e-4, np.abs(moved[:, 0] - want).max()
            assert np.abs(moved[:, 1]).max() < 0.05 and (moved[:, 2] == 0).all()                       # y follows the prey's sway; z stays
            assert abs(want[0] + 0.02 * 20 * 1.979) < 0.01 and abs(want[-1] + 0.02 * 20 * 1.183) < 0.01    # ~ lim(ep 10) and lim(ep 410)
        assert torch.equal(env.curr_episode_step[alive], torch.from_numpy(ep0).to(DEV)[alive] + k)
        if bool(fresh.any()):
            ids = fresh.nonzero().flatten()
            assert bool((env.curr_episode_step[ids] == 0).all()) and bool((env.predator_pos[ids, 2] == 0.3).all())
            assert bool((obs[ids, 0:9] == 100).all())
    got = first.cpu().numpy()
    assert (got > 0).all() and (np.abs(got - expect) <= 1).all(), (got.tolist(), expect.tolist())
    assert torch.isfinite(rew).all()


# ----------------------------------------------------------------------------- 6. env paths
GUARD = 0.15          # rad: as tests/test_gpu_game.py


def test_env_step_equals_its_parts_and_the_twin(tmp_path):
    """A calls ``step``; on B the test issues lg_game_pre -> low-level actor -> low-level step -> lg_pursuer_post by hand and checks the last
    against the twin from a snapshot of its inputs; A and B agree bit for bit at every step.  The twin's flags are undefined within the
    margins of tests/game_twin.py, so envs inside a margin at a step (few: they are counted) are left out of that step's twin comparison."""
    from legged_games_gym_amd import capi
    N = 64
    A, B = two_scripted(tmp_path, seed=7, reset_seed=70, n=N)
    p, q = unpack_params(B._P), unpack_pursuer(B._Q)
    assert q == {k: (float(F(v)) if isinstance(v, float) else v) for k, v in pt.pursuer_params().items()}          # the registered rule, as float32
    gen = torch.Generator().manual_seed(5)
    stream = torch.cuda.current_stream().cuda_stream
    compared, done_seen, negative = 0, 0, 0
    for k in range(12):
        cmd = (3.0 * torch.randn(N, 6, generator=gen)).to(DEV)
        ca, cb = cmd.clone(), cmd.clone()
        before = B.curr_episode_step.clone()
        A.step(ca)
        ll = B.ll_env
        bufs = B._bind_command(cb, B.obs_buf)
        capi.game_pre(B._P, bufs, stream)
        ll.step(B.ll_policy(ll.obs_buf))
        torch.cuda.synchronize()
        s = snapshot(B, cb)
        capi.pursuer_post(B._P, B._Q, bufs, B.predator_command.data_ptr(), ll.common_step_counter, stream)
        torch.cuda.synchronize()
        assert torch.equal(ca, cb)
        assert_same_state(A, B, k)
        assert_within_limit(B, before, k)
        want, info = pt.post(p, q, s, step=ll.common_step_counter)
        np.testing.assert_array_equal(B.predator_command.cpu().numpy().view(np.uint32), info["predator_command"].view(np.uint32))
        ok = ~(np.isnan(info["angle"]) | (np.abs(np.abs(info["angle"]) - F(p["half_fov"])) < 1e-3) | (np.abs(info["dist_xy"] - F(p["capture_dist"])) < 1e-4)
               | (info["rel_norm"] < 1e-3))
        pick = lambda d: {key: (v[:, ok] if key == "episode_sums" else v[ok]) for key, v in d.items() if isinstance(v, np.ndarray)}
        check_call(p, pick(s), pick(outputs(B)), pick(info), pick(want), extra_ulp=2)
        compared += int(ok.sum()); done_seen += int(want["reset_buf"].sum()); negative += int((info["lim"] < 0).sum())
    assert compared >= 0.95 * 12 * N and done_seen >= 8 and negative >= 12, (compared, done_seen, negative)


def policy_net():
    torch.manual_seed(11)
    net = torch.nn.Sequential(torch.nn.Linear(19, 64), torch.nn.ELU(), torch.nn.Linear(64, 6)).to(DEV)

    def policy(obs):
        with torch.no_grad():
            return 2.0 * torch.tanh(net(obs * 0.05))
    return policy


def test_graphed_step_equals_eager_steps(tmp_path):
    """``make_graphed_step`` (3 warm-up steps, then 8 replays of the five captured launches) equals 11 eager ``step`` calls."""
    A, B = two_scripted(tmp_path, seed=9, reset_seed=90)
    policy = policy_net()
    replay = A.make_graphed_step(policy, warmup=3)
    for _ in range(3):
        B.step(policy(B.obs_buf))
    resets = 0
    for k in range(8):
        before = B.curr_episode_step.clone()
        oa, _, ra, da, _ = replay()
        ob, _, rb, db, _ = B.step(policy(B.obs_buf))
        torch.cuda.synchronize()
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db), k
        assert_same_state(A, B, k)
        assert_within_limit(A, before, k)
        resets += int(da.sum())
    assert resets >= 8 and A.ll_env.common_step_counter == B.ll_env.common_step_counter
    assert float(A.predator_command.abs().max()) > 0


def test_step_policy_equals_step_fed_its_command(tmp_path):
    """A: ``step_policy`` (lg_game_act -> lg_step -> lg_pursuer_post).  B: ``step`` fed the unclipped sample A's actor launch produced."""
    from legged_games_gym_amd.rl import FusedActor
    A, B = two_scripted(tmp_path, seed=9, reset_seed=90)
    fa = FusedActor(high_level_actor(seed=6), DEV, seed=21)
    sample = torch.empty(A.num_envs, 6, device=DEV)
    resets = 0
    for k in range(10):
        before = A.curr_episode_step.clone()
        (ca, ma), (oa, _, ra, da, _) = A.step_policy(fa, sample=sample)
        fed = sample.clone()
        ob, _, rb, db, _ = B.step(fed)                                  # clips `fed` where it is
        torch.cuda.synchronize()
        assert torch.equal(ca, fed) and torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db), k
        assert_same_state(A, B, k)
        assert_within_limit(A, before, k)
        resets += int(da.sum())
    assert resets >= 8 and A.ll_env.common_step_counter == B.ll_env.common_step_counter


def test_graphed_policy_step_equals_eager_step_policy(tmp_path):
    """``make_graphed_policy_step`` (3 warm-up steps, then 8 replays of the three captured launches) equals 11 eager ``step_policy`` calls."""
    from legged_games_gym_amd.rl import FusedActor
    A, B = two_scripted(tmp_path, seed=9, reset_seed=90)
    ac = high_level_actor(seed=6)
    fa = FusedActor(ac, DEV, seed=21, step_counter=A.ll_env._sim.buf["step_counter"])
    fb = FusedActor(ac, DEV, seed=21, step_counter=B.ll_env._sim.buf["step_counter"])
    replay = A.make_graphed_policy_step(fa, warmup=3)
    for _ in range(3):
        B.step_policy(fb)
    resets = 0
    for k in range(8):
        before = B.curr_episode_step.clone()
        oa, _, ra, da, _ = replay()
        (cb, mb), (ob, _, rb, db, _) = B.step_policy(fb)
        torch.cuda.synchronize()
        ca, ma = fa.output_buffers(A.num_envs)
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db) and torch.equal(ca, cb) and torch.equal(ma, mb), k
        assert_same_state(A, B, k)
        assert_within_limit(A, before, k)
        resets += int(da.sum())
    assert resets >= 8 and A.ll_env.common_step_counter == B.ll_env.common_step_counter


@pytest.fixture
def scripted_registered():
    from legged_games_gym_amd.envs import a1_game, task_registry
    assert set(task_registry.task_classes) == LOCOMOTION_TASKS
    a1_game.register_scripted()
    try:
        yield task_registry
    finally:
        a1_game.unregister_scripted()
        assert set(task_registry.task_classes) == set(task_registry.env_cfgs) == set(task_registry.train_cfgs) == LOCOMOTION_TASKS


@pytest.mark.parametrize("device_rollout", [True, False])
def test_two_ppo_iterations_finish_with_finite_losses(tmp_path, monkeypatch, scripted_registered, device_rollout):
    """Through the registry and the runner: with ``device_rollout`` the rollout is ``step_policy`` captured into one graph, without it the
    generic VecEnv loop; the pursuer's kernel runs on both and its velocity stays within the limit of the env's episode step."""
    import legged_games_gym_amd.utils.task_registry as tr_mod
    from legged_games_gym_amd.utils import get_args
    reg = scripted_registered
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    monkeypatch.setattr(tr_mod, "LEGGED_GYM_ROOT_DIR", str(tmp_path))
    env_cfg, train_cfg = reg.get_cfgs("scripted_predator_game")
    env_cfg.terrain.mesh_type, env_cfg.env.ll_policy_path = "plane", ckpt
    if device_rollout:
        train_cfg.runner.device_rollout = True                          # a runner key, set on this registration only
    args = get_args(["--task", "scripted_predator_game", "--num_envs", "64", "--headless", "--sim_device", DEV, "--rl_device", DEV])
    env, _ = reg.make_env("scripted_predator_game", args)
    runner, _ = reg.make_alg_runner(env, "scripted_predator_game", args)
    assert type(env).__name__ == "ScriptedPredatorGame" and (runner._fused is not None) == device_rollout and runner._game_rollout == device_rollout
    losses, posts, graphs = [], [], []
    update, post, build = runner.alg.update, env._post, runner._try_build_graphed_rollout
    runner.alg.update = lambda *a, **k: losses.append(update(*a, **k)) or losses[-1]
    env._post = lambda *a, **k: posts.append(1) or post(*a, **k)
    runner._try_build_graphed_rollout = lambda: graphs.append(build()) or graphs[-1]
    runner.learn(num_learning_iterations=2, init_at_random_ep_len=True)
    torch.cuda.synchronize()
    assert len(losses) == 2 and all(math.isfinite(float(v)) for pair in losses for v in pair)
    # lg_pursuer_post was issued from Python once per step of two rollouts: the two eager ones, or the warm-up and the captured one
    assert len(posts) == 2 * runner.num_steps_per_env if device_rollout else len(posts) >= 2 * runner.num_steps_per_env
    assert len(graphs) == 1 and (graphs[0] is not None) == device_rollout    # the rollout was captured into one graph, as for high_level_game
    assert torch.isfinite(env.obs_buf).all() and torch.isfinite(env.rew_buf).all() and torch.isfinite(env.predator_pos).all()
    lim_max = float(pt.speed_limit(unpack_pursuer(env._Q), np.array([0]))[0])
    assert float(env.predator_command.abs().max()) <= lim_max and float(env.predator_command.abs().max()) > 0
    assert str(tmp_path / "logs" / "scripted_predator_game") in runner.log_dir
