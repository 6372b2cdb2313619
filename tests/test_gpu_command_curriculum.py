"""commands.curriculum on the fast paths (graphed steps, rolled rollouts, the runner's captured rollout) against the eager steps with
the host rule (reference legged_robot.py:159-168, rule :471-483), step by step across the ticks.  Short episodes (max_episode_length 10)
put curriculum ticks INSIDE a segment.  What a tick does is set up from the host, identically on both sides: before the step or segment
that holds it, the tracking sums of all envs are raised far above the rule's threshold (the tick's reset envs started their episode
before that write: lin_vel_x widens by 0.5, up to max_curriculum = 1.1, or stays at it) or zeroed (the rule is false); a tick whose
reset envs earned their sums on their own (a robot with random initial velocities over 0.2 s episodes stays below 80 %) leaves the
range unchanged too.  Every test checks that widening and non-widening ticks occurred."""
import copy
import csv
import glob
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

MAX_CURRICULUM = 1.1


def _cfgs(task, episode_length_s):
    from legged_games_gym_amd.envs import task_registry
    env_cfg, train_cfg = task_registry.get_cfgs(task)
    env_cfg, train_cfg = copy.deepcopy(env_cfg), copy.deepcopy(train_cfg)
    env_cfg.commands.curriculum, env_cfg.commands.max_curriculum = True, MAX_CURRICULUM
    env_cfg.commands.ranges.lin_vel_x = [-0.1, 0.1]
    env_cfg.commands.ranges.lin_vel_y = [-0.1, 0.1]
    env_cfg.env.episode_length_s = episode_length_s
    return env_cfg, train_cfg


def _make(task, N, episode_length_s=0.2):
    """A curriculum env with every env at a random point of its episode (resets on every step, so every tick has some)."""
    from legged_games_gym_amd.envs import task_registry
    from legged_games_gym_amd.utils import get_args
    env_cfg, _ = _cfgs(task, episode_length_s)
    args = get_args(["--task", task, "--num_envs", str(N), "--headless", "--sim_device", "cuda:0", "--rl_device", "cuda:0"])
    torch.manual_seed(0)
    env, _ = task_registry.make_env(task, args, env_cfg=env_cfg)
    env.reset()
    M = int(env.max_episode_length)
    env.episode_length_buf[:] = torch.randint(0, M, (N,), generator=torch.Generator().manual_seed(5)).to(env.device)
    torch.cuda.synchronize()
    return env


def _standing_actor(env, std=0.05):
    """A fused actor whose mean is 0 (last layer zeroed) with a small std: the robot stands, commands of 0 are tracked."""
    from legged_games_gym_amd.envs import task_registry
    from legged_games_gym_amd.rl import ActorCritic, FusedActor
    from legged_games_gym_amd.utils.helpers import class_to_dict
    _, train_cfg = task_registry.get_cfgs("anymal_c_flat")
    torch.manual_seed(3)
    ac = ActorCritic(env.num_obs, env.num_obs, env.num_actions, **class_to_dict(train_cfg.policy)).to("cuda")
    with torch.no_grad():
        ac.actor[-1].weight.zero_()
        ac.actor[-1].bias.zero_()
        ac.std.fill_(std)
    return FusedActor(ac, "cuda:0", seed=11)


def _range(env):
    env.sync_command_ranges()
    return tuple(float(v) for v in env.command_ranges["lin_vel_x"])


class _Ticks:
    """Eager-side record of the curriculum ticks (counter % max_episode_length == 0 with resets): widening or not."""
    def __init__(self, env):
        self.env, self.widened, self.kept = env, 0, 0
        self.r = _range(env)

    def after_step(self, dones):
        env = self.env
        r = tuple(float(v) for v in env.command_ranges["lin_vel_x"])
        if env.common_step_counter % int(env.max_episode_length) == 0 and bool(dones.any()):
            if r != self.r:
                assert r[1] > self.r[1] and r[0] < self.r[0]
                self.widened += 1
            else:
                self.kept += 1
        else:
            assert r == self.r
        self.r = r

    def check(self):
        assert self.widened >= 1 and self.kept >= 1, (self.widened, self.kept)


def _force_tracking(env):
    """Make the rule fire on the next tick: the reset envs' mean tracking sum well above 80 % of its maximum (same write on both sides)."""
    env.episode_sums["tracking_lin_vel"][:] = env.reward_scales["tracking_lin_vel"] * env.max_episode_length


STATE = ("root_states", "dof_state", "episode_length_buf", "commands", "last_actions")


def _compare_states(a, b, tol=2e-4):
    for k in a:
        if not a[k].dtype.is_floating_point:
            assert torch.equal(a[k], b[k]), k
        else:
            err = float((a[k].double() - b[k].double()).abs().max())
            assert err < tol, (k, err)


def _close(a, b, tol):
    err = float((a.double() - b.double()).abs().max())
    assert err < tol, err


def test_rolled_rollout_ticks_like_the_eager_steps():
    T, N = 44, 256                               # max_episode_length 10: ticks at 10, 20, 30, 40 inside the one segment
    env = _make("anymal_c_flat", N)
    actor = _standing_actor(env)
    ticks = _Ticks(env)
    obs, rew, dones, touts, acts = [], [], [], [], []
    _force_tracking(env)                         # tick 10 widens (its reset envs started before this write), the later ones earn their own
    with torch.inference_mode():
        for _ in range(T):
            (a, _), (o, _, r, d, _) = env.step_policy(actor)
            obs.append(o.clone()); rew.append(r.clone()); dones.append(d.clone()); touts.append(env.time_out_buf.clone()); acts.append(a.clone())
            ticks.after_step(d)
    torch.cuda.synchronize()
    ticks.check()
    eager_state = {k: env._sim.buf[k].clone() for k in STATE}
    eager_range, eager_max = _range(env), env.extras["episode"]["max_command_x"]
    assert isinstance(eager_max, float)

    env2 = _make("anymal_c_flat", N)
    actor2 = _standing_actor(env2)
    _force_tracking(env2)
    with torch.inference_mode():
        st = env2.rollout_policy(actor2, T)
    torch.cuda.synchronize()
    assert env2.common_step_counter == env.common_step_counter
    assert torch.equal(st["dones"], torch.stack(dones)) and torch.equal(st["time_outs"], torch.stack(touts))
    _close(st["obs"][1:], torch.stack(obs), 1e-2)
    _close(st["rew"], torch.stack(rew), 1e-3)
    _close(st["actions"], torch.stack(acts), 1e-3)
    _compare_states({k: env2._sim.buf[k] for k in STATE}, eager_state, tol=1e-3)
    _close(env2._sim.buf["commands"], eager_state["commands"], 1e-5)
    mx = env2.extras["episode"]["max_command_x"]
    assert torch.is_tensor(mx) and mx.dim() == 0 and float(mx) == eager_max
    assert _range(env2) == eager_range and eager_range[1] > 0.1


def _steer(env, counter):
    """Set the tracking sums before the step / segment that holds tick `counter` (same write on both sides): ticks 1, 3, 4 (x
    max_episode_length) get sums far above the rule's threshold -- widen, widen to max_curriculum, saturated (rule true, range kept) --
    tick 2 gets zero sums: the rule is false there (the reset envs' own few steps stay below 80 % of an episode's maximum)."""
    if (counter // int(env.max_episode_length)) % 4 == 2:
        env.episode_sums["tracking_lin_vel"][:] = 0.0
    else:
        _force_tracking(env)


def _record(env, obs):
    """Per-step outputs that a tick changes: observations (slots 9-11 are the commands), rewards, resets, commands, the device range
    and extras["episode"] as published."""
    return {"obs": obs.clone(), "rew": env.rew_buf.clone(), "dones": env.reset_buf.clone(), "commands": env.commands.clone(),
            "range": env._sim.buf["cmd_range"].clone(), "means": env._sim.buf["episode_means"].clone()}


def _compare_steps(eager, fast, what):
    assert len(eager) == len(fast)
    for t, (a, b) in enumerate(zip(eager, fast)):
        assert torch.equal(a["dones"], b["dones"]), (what, t)
        assert torch.equal(a["range"], b["range"]), (what, t, a["range"].tolist(), b["range"].tolist())
        for k, tol in (("obs", 1e-5), ("rew", 1e-5), ("commands", 1e-6)):
            err = float((a[k].double() - b[k].double()).abs().max())
            assert err < tol, (what, t, k, err)
        err = float(((a["means"].double() - b["means"].double()).abs() / a["means"].double().abs().clamp(min=1e-3)).max())
        assert err < 1e-4, (what, t, "episode_means", err)


def test_graphed_rollout_replays_tick_like_the_eager_steps():
    T, N, W = 12, 256, 1                         # warm-up segment + 3 replays = 48 steps: ticks at 10, 20, 30, 40, three inside replays
    segs, ticks = [], None
    for rolled in (False, True):
        env = _make("anymal_c_flat", N)
        actor = _standing_actor(env)
        out = []
        with torch.inference_mode():             # the sums are set before every segment for the tick inside it (_steer)
            if rolled:
                _steer(env, env.common_step_counter + T)
                replay, st = env.make_graphed_rollout(actor, T, warmup=W)
                for i in range(3 + 1):
                    if i:
                        _steer(env, env.common_step_counter + T)
                        replay()
                    torch.cuda.synchronize()
                    out.append({k: st[k].clone() for k in ("obs", "actions", "rew", "dones", "time_outs")}
                               | {"commands": env.commands.clone(), "range": env._sim.buf["cmd_range"].clone()})
            else:
                ticks = _Ticks(env)
                seg = None
                for i in range((W + 3) * T):
                    if i % T == 0:
                        _steer(env, env.common_step_counter + T)
                        seg = {"obs": [env.obs_buf.clone()], "actions": [], "rew": [], "dones": [], "time_outs": []}
                    (a, _), (o, _, r, d, _) = env.step_policy(actor)
                    ticks.after_step(d)
                    seg["obs"].append(o.clone()); seg["actions"].append(a.clone()); seg["rew"].append(r.clone())
                    seg["dones"].append(d.clone()); seg["time_outs"].append(env.time_out_buf.clone())
                    if i % T == T - 1:
                        out.append({k: torch.stack(v) for k, v in seg.items()}
                                   | {"commands": env.commands.clone(), "range": torch.tensor(env.command_ranges["lin_vel_x"], dtype=torch.float64, device=env.device)})
                assert (ticks.widened, ticks.kept) == (2, 2), (ticks.widened, ticks.kept)
        torch.cuda.synchronize()
        segs.append((out, env.common_step_counter, float(env.extras["episode"]["max_command_x"])))
    (a, ca, ma), (b, cb, mb) = segs
    assert ca == cb and ma == mb == MAX_CURRICULUM
    for s, (x, y) in enumerate(zip(a, b)):                 # segment by segment, step by step
        assert torch.equal(x["dones"], y["dones"]) and torch.equal(x["time_outs"], y["time_outs"]), s
        assert torch.equal(x["range"], y["range"]), (s, x["range"].tolist(), y["range"].tolist())
        for k, tol in (("obs", 1e-3), ("actions", 1e-3), ("rew", 1e-3), ("commands", 1e-5)):
            err = float((x[k].double() - y[k].double()).abs().max())
            assert err < tol, (s, k, err)


def _graphed_vs_eager(task, N, make_replay, eager_step, warmup=3, steps=44, episode_length_s=0.2):
    """A one-step graph replayed against eager steps, compared after EVERY step (observations incl. the command slots, rewards, resets,
    commands, range, extras["episode"]).  The sums are steered before each tick (_steer): widen, rule false, widen to max_curriculum,
    saturated."""
    runs = []
    for graphed in (False, True):
        env = _make(task, N, episode_length_s)
        M = int(env.max_episode_length)
        out = []
        with torch.inference_mode():
            if graphed:
                c0 = env.common_step_counter
                replay = make_replay(env)                      # (runs its warm-up steps)
                assert (c0 + warmup) // M == c0 // M           # no tick among them
                while env.common_step_counter < c0 + steps:
                    _steer(env, env.common_step_counter + 1)
                    obs = replay()[0]
                    out.append(_record(env, obs))
            else:
                ticks = _Ticks(env)
                for i in range(steps):
                    _steer(env, env.common_step_counter + 1)
                    obs, _, _, d, _ = eager_step(env)
                    ticks.after_step(d)
                    rec = _record(env, obs)
                    rec["range"] = torch.tensor(env.command_ranges["lin_vel_x"], dtype=torch.float64, device=env.device)
                    if i >= warmup:
                        out.append(rec)
                assert (ticks.widened, ticks.kept) == (2, 2), (ticks.widened, ticks.kept)
        torch.cuda.synchronize()
        runs.append((out, env.common_step_counter, float(env.extras["episode"]["max_command_x"])))
    (a, ca, ma), (b, cb, mb) = runs
    assert ca == cb and ma == mb == MAX_CURRICULUM
    _compare_steps(a, b, task)


def test_graphed_policy_step_ticks_like_the_eager_steps():
    holder = {}

    def make(env):
        holder["actor"] = _standing_actor(env)
        return env.make_graphed_policy_step(holder["actor"], warmup=3)

    def eager(env):
        if "eager_actor" not in holder:
            holder["eager_actor"] = _standing_actor(env)
        return env.step_policy(holder["eager_actor"])[1]
    _graphed_vs_eager("anymal_c_flat", 256, make, eager)


@pytest.mark.parametrize("task", ["anymal_c_flat", "anymal_c_rough", "cassie"])
def test_graphed_step_ticks_like_the_eager_steps(task):
    def make(env):
        act = torch.zeros(env.num_envs, env.num_actions, device=env.device)
        return env.make_graphed_step(lambda obs: act, warmup=3)

    def eager(env):
        return env.step(torch.zeros(env.num_envs, env.num_actions, device=env.device))
    _graphed_vs_eager(task, 256, make, eager)


def test_runner_keeps_the_graphed_rolled_rollout_and_logs_a_growing_max_command_x(tmp_path, capsys):
    from legged_games_gym_amd.envs import task_registry
    from legged_games_gym_amd.utils import get_args
    env_cfg, train_cfg = _cfgs("anymal_c_flat", 0.5)          # max_episode_length 25: one tick in every 24-step iteration
    train_cfg.policy.init_noise_std = 0.05
    args = get_args(["--task", "anymal_c_flat", "--num_envs", "256", "--headless", "--sim_device", "cuda:0", "--rl_device", "cuda:0"])
    torch.manual_seed(0)
    env, _ = task_registry.make_env("anymal_c_flat", args, env_cfg=env_cfg)
    runner, _ = task_registry.make_alg_runner(env, "anymal_c_flat", args, train_cfg=train_cfg, log_root=str(tmp_path))
    with torch.no_grad():                                      # a standing robot: it tracks the zero commands of the first ranges
        runner.alg.actor_critic.actor[-1].weight.zero_()
        runner.alg.actor_critic.actor[-1].bias.zero_()
    runner._fused.sync_device()
    update = runner.alg.update

    def update_then_raise_the_sums():                         # between iterations: the next iteration's tick widens until saturation
        out = update()
        _force_tracking(env)
        return out
    runner.alg.update = update_then_raise_the_sums
    _force_tracking(env)
    runner.learn(6, init_at_random_ep_len=True)
    out = capsys.readouterr().out
    assert "graphed rollout unavailable" not in out and "torch policy in the rollout" not in out
    assert runner._rolled is True
    rows = list(csv.DictReader(open(glob.glob(os.path.join(str(tmp_path), "**", "progress.csv"), recursive=True)[0])))
    mx = [float(r["Episode/max_command_x"]) for r in rows]
    assert len(mx) == 6 and all(b >= a for a, b in zip(mx, mx[1:]))
    assert mx[-1] > mx[0] > 0.1                                 # widening ticks inside logged iterations
    # ... and saturated two iterations (48 steps, at least one tick with resets) before the end: a tick that cannot widen
    full = [abs(v - MAX_CURRICULUM) < 1e-6 for v in mx]
    assert full[-1] and full.index(True) < 4, mx
    assert _range(env)[1] == MAX_CURRICULUM
