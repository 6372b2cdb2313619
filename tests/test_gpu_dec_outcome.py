"""-m gpu: the outcome statistics of the decentralised game -- ``lg_dec_outcome_post`` (include/legged_dec_game_outcome.h) writes what
``lg_dec_game_post`` writes, bit for bit, and counts exactly what the NumPy twin counts (tests/dec_outcome_twin.py); the state and the totals
carried over consecutive launches and graph replays; every step path of the env with the switch off and on; the runner's logs;
``play_outcomes`` and the checkpoint cross-play.  Nothing here reads outside the tree."""
import copy
import csv
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import dec_game_twin as dt
from tests import dec_outcome_fixtures as of
from tests import dec_outcome_twin as ot
from tests.test_gpu_dec_game import STATE, dec_runner, device_post, fused_pair, make_dec, pack_params
from tests.test_gpu_game import place_ahead, write_ll_checkpoint

pytestmark = pytest.mark.gpu
F = np.float32
DEV = "cuda:0"
KEYS = tuple(f"outcome_{k}" for k in ot.MEANS)
PLAIN_KEYS = {"rew_pred_pursuit", "rew_prey_evasion"}
PER_ENV = ("root_states", "dof_pos", "dof_vel", "predator_pos", "obs_prey", "obs_pred", "rew_prey", "rew_pred", "reset_buf", "time_out_buf", "curr_episode_step",
           "episode_length_buf", "episode_sums")


# ----------------------------------------------------------------------------- the kernel without an env
class Launcher:
    """Device buffers of ``calls`` consecutive ``lg_dec_outcome_post`` launches on ``n`` envs: ONE set of state buffers, rewritten in place
    by every launch (as in an env), and per-call inputs (predator command, low-level reward / resets / time-outs, step counter), so that
    the launches can also be captured into a graph."""

    def __init__(self, state, calls):
        from legged_games_gym_amd import capi
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        self.calls, self.n = calls, state["root_states"].shape[0]
        n = self.n
        self.t = {k: up(state[k]) for k in ("root_states", "predator_pos", "obs_prey", "curr_episode_step", "episode_length_buf", "episode_sums", "episode_means",
                                            "env_origins")}
        self.t["dof"] = up(np.stack((state["dof_pos"], state["dof_vel"]), axis=-1).astype(F))
        assert self.t["curr_episode_step"].dtype == torch.int64 and self.t["obs_prey"].shape == (n, 16) and self.t["episode_sums"].shape == (3, n)
        self.t["obs_pred"], self.t["rew_prey"], self.t["rew_pred"] = torch.full((n, 3), -3.0, device=DEV), torch.full((n,), -3.0, device=DEV), torch.full((n,), -3.0, device=DEV)
        self.t["reset_buf"], self.t["time_out_buf"] = torch.zeros(n, dtype=torch.bool, device=DEV), torch.ones(n, dtype=torch.bool, device=DEV)
        self.extras_accum, self.extras_ticket = torch.zeros(4, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        self.accum, self.totals = torch.zeros(6, dtype=torch.int64, device=DEV), torch.zeros(6, dtype=torch.int64, device=DEV)
        self.means = torch.zeros(5, device=DEV)
        self.per_call = []
        for c in calls:
            d = dict(command_pred=up(c["command_pred"]), ll_rew=up(c["ll_rew"]), ll_reset=up(np.asarray(c["ll_reset"], bool)),
                     ll_time_out=up(np.asarray(c["ll_time_out"], bool)), counter=torch.tensor([c["step"]], dtype=torch.int64, device=DEV))
            assert d["ll_reset"].element_size() == 1 and d["ll_time_out"].element_size() == 1 and d["command_pred"].dtype == torch.float32 and d["ll_rew"].dtype == torch.float32
            t = self.t
            d["B"] = capi.dec_game_buffers({"command_pred": d["command_pred"].data_ptr(), "ll_root_states": t["root_states"].data_ptr(), "ll_dof_state": t["dof"].data_ptr(),
                                            "ll_env_origins": t["env_origins"].data_ptr(), "ll_rew_buf": d["ll_rew"].data_ptr(), "ll_reset_buf": d["ll_reset"].data_ptr(),
                                            "ll_step_counter": d["counter"].data_ptr(), "predator_pos": t["predator_pos"].data_ptr(), "obs_prey": t["obs_prey"].data_ptr(),
                                            "obs_pred": t["obs_pred"].data_ptr(), "rew_prey": t["rew_prey"].data_ptr(), "rew_pred": t["rew_pred"].data_ptr(),
                                            "reset_buf": t["reset_buf"].data_ptr(), "time_out_buf": t["time_out_buf"].data_ptr(),
                                            "curr_episode_step": t["curr_episode_step"].data_ptr(), "episode_length_buf": t["episode_length_buf"].data_ptr(),
                                            "episode_sums": t["episode_sums"].data_ptr(), "episode_means": t["episode_means"].data_ptr(),
                                            "extras_accum": self.extras_accum.data_ptr(), "extras_ticket": self.extras_ticket.data_ptr()})
            d["O"] = capi.dec_outcome_buffers({"ll_time_out_buf": d["ll_time_out"].data_ptr(), "accum": self.accum.data_ptr(), "means": self.means.data_ptr(),
                                               "totals": self.totals.data_ptr()})
            d["P"] = pack_params(dict(c["p"], num_envs=n))
            self.per_call.append(d)

    def launch(self, k, counter_on_device):
        from legged_games_gym_amd import capi
        d = self.per_call[k]
        capi.dec_outcome_post(d["P"], d["B"], d["O"], -1 if counter_on_device else self.calls[k]["step"], torch.cuda.current_stream().cuda_stream)

    def state(self):
        """The carried state as NumPy arrays (synchronises)."""
        torch.cuda.synchronize()
        out = {k: self.t[k].cpu().numpy() for k in of.CARRIED if k not in ("dof_pos", "dof_vel")}
        out["dof_pos"], out["dof_vel"] = self.t["dof"][..., 0].cpu().numpy(), self.t["dof"][..., 1].cpu().numpy()
        return out

    def outputs(self):
        out = self.state()
        out.update({k: self.t[k].cpu().numpy() for k in ("obs_pred", "rew_prey", "rew_pred", "reset_buf", "time_out_buf")})
        return out

    def stats(self):
        """-> (accum, extras_accum, ticket, means, totals) (synchronises)."""
        torch.cuda.synchronize()
        return self.accum.cpu().numpy(), self.extras_accum.cpu().numpy(), int(self.extras_ticket[0]), self.means.cpu().numpy(), self.totals.cpu().numpy()

    def restore(self, state):
        for k in of.CARRIED:
            if k not in ("dof_pos", "dof_vel"):
                self.t[k].copy_(torch.from_numpy(np.ascontiguousarray(state[k])))
        self.t["dof"].copy_(torch.from_numpy(np.stack((state["dof_pos"], state["dof_vel"]), axis=-1).astype(F)))


def ulps(a, b):
    """Distance of two float32 arrays in units in the last place of ``b``."""
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(b), np.finfo(F).tiny).astype(F)).astype(np.float64)


def int_view(a):
    return a.view(np.uint8) if a.dtype == bool else a.view(np.uint32 if a.itemsize == 4 else np.uint64)


CASES = [(n, t, False) for n in of.SIZES for t in of.TERMINATIONS] + [(1, 0.0, True)]


@pytest.mark.parametrize("n,termination,forced", CASES)
def test_same_step_bit_for_bit_and_exact_counts(n, termination, forced):
    """One launch of ``lg_dec_outcome_post`` against one of ``lg_dec_game_post`` on the same inputs: every per-env array either writes as
    integer views; the episode means bit-equal where one workgroup fixes the order of the float sum (n <= 256), within
    ``dec_game_twin.means_bound`` of the twin above (float atomics arrive in any order in both kernels).  Then the statistics of that launch
    against the twin: the six integers exactly, both accumulators and the ticket back at zero, the five means within 3 ulp of the twin's
    float32 quotient (the library's division is the 2.5-ulp one, DESIGN.md section 5 "The division").  A launch without a done env leaves
    means and totals at zero.  The extra n = 1 case is the one with exactly one done env (the seeded n = 1 draws have none)."""
    c = of.single_done_case() if forced else of.case(n, termination)
    s, odd = c["s"], bool(n % 2)
    plain = device_post(c["p"], s, c["step"], counter_on_device=odd)
    call = dict(p=c["p"], step=c["step"], command_pred=s["command_pred"], ll_rew=s["ll_rew"], ll_reset=s["ll_reset"], ll_time_out=c["ll_time_out"])
    L = Launcher(s, [call])
    L.launch(0, counter_on_device=odd)
    got = L.outputs()
    for k in PER_ENV:
        a, b = got[k], plain[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        np.testing.assert_array_equal(int_view(a), int_view(b), err_msg=k)
    d = L.per_call[0]
    assert np.array_equal(d["command_pred"].cpu().numpy(), s["command_pred"]) and int(d["counter"][0]) == c["step"]                 # inputs are left alone
    assert np.array_equal(d["ll_reset"].cpu().numpy(), np.asarray(s["ll_reset"], bool)) and np.array_equal(d["ll_time_out"].cpu().numpy(), c["ll_time_out"])
    np.testing.assert_array_equal(got["reset_buf"].astype(bool), c["flags"]["done"])
    if n <= 256:
        np.testing.assert_array_equal(got["episode_means"].view(np.uint32), plain["episode_means"].view(np.uint32))
    else:
        bound = dt.means_bound(c["p"], c["info"])
        dm = np.abs(got["episode_means"].astype(np.float64) - c["want"]["episode_means"].astype(np.float64))
        print(f"n {n}: episode means off the twin by {dm.tolist()}, bound {bound.tolist()}")
        assert (dm <= bound).all(), (dm, bound)
    accum, extras_accum, ticket, means, totals = L.stats()
    np.testing.assert_array_equal(totals, c["counts"])
    assert not accum.any() and not extras_accum.any() and ticket == 0
    worst = float(ulps(means, c["means"]).max())
    print(f"n {n} termination {termination} forced {forced}: counts {totals.tolist()}, means off by at most {worst:.2f} ulp")
    if int(c["counts"][0]) == 0:
        assert not means.any() and not totals.any()
        np.testing.assert_array_equal(got["episode_means"].view(np.uint32), s["episode_means"].view(np.uint32))
    else:
        assert forced or n > 1
    assert worst <= 3.0, (means.tolist(), c["means"].tolist())


def test_state_and_totals_carried_over_four_launches_and_graph_replays():
    """Four consecutive launches at 257 envs on one set of buffers, the twin fed the state the device left: ``totals`` adds up call by call,
    the call without a done env leaves ``means`` and ``totals`` bit-identical, both accumulators and the ticket read zero after every call.
    The step counter is passed by value on even calls and read from the device on odd ones.  Then the same four launches captured into one
    graph and replayed twice from the restored inputs: twice the totals, the same final state."""
    p, state0, calls = of.sequence_inputs()
    L = Launcher(state0, calls)
    running, prev_means, per_call = np.zeros(6, np.int64), np.zeros(5, F), []
    for k, c in enumerate(calls):
        before = L.state()
        s = dict(before, env_origins=state0["env_origins"], command_pred=c["command_pred"], ll_rew=c["ll_rew"], ll_reset=c["ll_reset"])
        _, info = dt.post(c["p"], s, step=c["step"])
        assert float(np.min(np.abs(info["dist_xy"] - F(c["p"]["capture_dist"])))) >= 1e-4          # no env near the one threshold the counts depend on
        f, cnt, want_means = ot.outcome(info, c["ll_reset"], c["ll_time_out"], before["curr_episode_step"], prev_means)
        L.launch(k, counter_on_device=bool(k % 2))
        accum, extras_accum, ticket, means, totals = L.stats()
        running = running + cnt
        np.testing.assert_array_equal(totals, running, err_msg=f"call {k}")
        assert not accum.any() and not extras_accum.any() and ticket == 0, k
        np.testing.assert_array_equal(L.t["reset_buf"].cpu().numpy().astype(bool), f["done"])
        if k == of.SEQ_QUIET:
            assert int(cnt[0]) == 0 and not f["done"].any()
            np.testing.assert_array_equal(means.view(np.uint32), prev_means.view(np.uint32))
        else:
            assert int(cnt[0]) > 0
            assert float(ulps(means, want_means).max()) <= 3.0, (k, means.tolist(), want_means.tolist())
        prev_means = means
        per_call.append(cnt)
    assert running[0] == sum(int(c[0]) for c in per_call) > 50 and all(int(v) > 0 for v in running), running.tolist()
    final, final_means = L.state(), L.stats()[3]

    L.restore(state0)
    L.totals.zero_()
    L.means.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for k in range(len(calls)):
            L.launch(k, counter_on_device=bool(k % 2))
    for rep in range(2):
        L.restore(state0)
        graph.replay()
        accum, extras_accum, ticket, means, totals = L.stats()
        np.testing.assert_array_equal(totals, (rep + 1) * running, err_msg=f"replay {rep}")
        assert not accum.any() and not extras_accum.any() and ticket == 0
        np.testing.assert_array_equal(means.view(np.uint32), final_means.view(np.uint32))
        now = L.state()
        for key in of.CARRIED:
            if key != "episode_means":                                          # (a float sum over two workgroups: its order is not fixed)
                np.testing.assert_array_equal(now[key], final[key], err_msg=f"replay {rep}: {key}")


# ----------------------------------------------------------------------------- the env, every path
def two_envs(tmp_path, seed, reset_seed, n=64):
    """Two identically seeded envs, the second with the outcome statistics on; the capture distance raised from the registered 0.5 m to
    2.5 m in both (as tests/test_gpu_outcome.py)."""
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    A, B = make_dec(ckpt, n, seed=seed), make_dec(ckpt, n, seed=seed)
    B.enable_outcome_stats()
    for env in (A, B):
        env.capture_dist = 2.5
        env.set_command_ranges()                  # re-packs lg_dec_game_params
        torch.manual_seed(reset_seed)             # reset_idx from the host draws from torch's generator
        env.reset()
    assert set(A.extras) == set(B.extras) == {"time_outs", "episode"}
    assert set(A.extras["episode"]) == PLAIN_KEYS and set(B.extras["episode"]) == PLAIN_KEYS | set(KEYS)
    return A, B


def arrange(env):
    """So that captures, game time-outs and low-level time-outs each occur within the 40 steps (after a capture's warm-up steps): 16
    predators 1.5 m ahead of their prey, 8 game episodes 3 steps from their limit, 8 low-level episodes 4 steps from theirs, and spread
    episode steps."""
    n = env.num_envs
    env.curr_episode_step[:] = torch.arange(n, device=DEV) * (900 // n)
    place_ahead(env, torch.arange(32, 48, device=DEV), 1.5)
    env.episode_length_buf[16:24] = int(env.max_episode_length) - 3
    env.ll_env.episode_length_buf[:8] = int(env.ll_env.max_episode_length) - 4


def assert_same(A, B, k):
    for name in STATE:
        assert torch.equal(getattr(A, name), getattr(B, name)), (k, name)
    for name in ("root_states", "dof_state", "obs_buf", "commands"):
        assert torch.equal(getattr(A.ll_env, name), getattr(B.ll_env, name)), (k, name)


def torch_policies():
    torch.manual_seed(11)
    net_p = torch.nn.Sequential(torch.nn.Linear(3, 32), torch.nn.ELU(), torch.nn.Linear(32, 2)).to(DEV)
    net_y = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.ELU(), torch.nn.Linear(32, 4)).to(DEV)

    def policy(net):
        def act(obs):
            with torch.no_grad():
                return 2.0 * torch.tanh(net(obs * 0.05))
        return act
    return policy(net_p), policy(net_y)


@pytest.mark.parametrize("path", ["step", "graphed_step", "step_policy", "graphed_policy_step", "view_step_policy"])
def test_env_paths_are_unchanged_by_the_switch_and_count_every_episode(tmp_path, path):
    """40 steps on one step path of two identically seeded envs, statistics off (A) and on (B): the state bit-equal at every step; A's
    extras keep the plain task's keys, B's additionally hold the five device scalars; B's totals equal the summed ``reset_buf``, the summed
    (pre-step ``curr_episode_step`` + 1) of the done envs, the summed ``time_out_buf`` and the low-level env's own ``reset_buf`` /
    ``time_out_buf`` sums."""
    A, B = two_envs(tmp_path, seed=9, reset_seed=90)
    if path in ("step", "graphed_step"):
        pol_p, pol_y = torch_policies()
        if path == "step":
            step_a = lambda: A.step(pol_p(A.obs_buf_pred), pol_y(A.obs_buf_prey))[7]
            step_b = lambda: B.step(pol_p(B.obs_buf_pred), pol_y(B.obs_buf_prey))[7]
        else:
            ra, rb = A.make_graphed_step(pol_p, pol_y, warmup=3), B.make_graphed_step(pol_p, pol_y, warmup=3)
            step_a, step_b = (lambda: ra()[7]), (lambda: rb()[7])
    else:
        graphed = path == "graphed_policy_step"
        (pa, ya), (pb, yb) = fused_pair(A if graphed else None), fused_pair(B if graphed else None)
        if path == "step_policy":
            step_a, step_b = (lambda: A.step_policy(pa, ya)[2][7]), (lambda: B.step_policy(pb, yb)[2][7])
        elif graphed:
            ra, rb = A.make_graphed_policy_step(pa, ya, warmup=3), B.make_graphed_policy_step(pb, yb, warmup=3)
            step_a, step_b = (lambda: ra()[7]), (lambda: rb()[7])
        else:
            va, vb = A.agent_view("prey", pa), B.agent_view("prey", pb)
            step_a, step_b = (lambda: va.step_policy(ya)[1][4]), (lambda: vb.step_policy(yb)[1][4])
    for env in (A, B):
        arrange(env)
    B.reset_outcome_totals()                                   # (the reset and the warm-up steps of a capture were counted too)
    assert_same(A, B, -1)
    zero = lambda: torch.zeros((), dtype=torch.int64, device=DEV)
    episodes, steps, timed_out, fell, ll_timed_out = zero(), zero(), zero(), zero(), zero()
    ll_reset, ll_time_out = B.ll_env._sim.buf["reset_buf"], B.ll_env._sim.buf["time_out_buf"]
    for k in range(40):
        before = B.curr_episode_step.clone()
        extras_a, extras_b = step_a(), step_b()
        assert_same(A, B, k)
        assert extras_a is A.extras and set(A.extras) == {"time_outs", "episode"} and set(A.extras["episode"]) == PLAIN_KEYS
        assert extras_b is B.extras and set(B.extras["episode"]) == PLAIN_KEYS | set(KEYS)
        episodes += B.reset_buf.sum()
        steps += ((before + 1) * B.reset_buf).sum()
        timed_out += B.time_out_buf.sum()
        fell += (ll_reset.bool() & ~ll_time_out.bool()).sum()
        ll_timed_out += (ll_reset.bool() & ll_time_out.bool()).sum()
        assert bool((B.reset_buf | ~ll_reset.bool()).all()) and bool((B.reset_buf | ~B.time_out_buf).all())      # either ends the game's episode
    torch.cuda.synchronize()
    totals = B.outcome_totals()
    print(f"{path}: {totals}")
    assert tuple(totals) == ot.COUNTS and all(isinstance(v, int) for v in totals.values())
    assert totals["episodes"] == int(episodes) and totals["steps"] == int(steps) and totals["timed_out"] == int(timed_out)
    assert totals["fell"] == int(fell) and totals["ll_timed_out"] == int(ll_timed_out)
    assert totals["captured"] >= 16 and totals["timed_out"] > 0 and totals["ll_timed_out"] > 0
    assert totals["captured"] + totals["timed_out"] + totals["fell"] + totals["ll_timed_out"] >= totals["episodes"] >= 16
    for key in KEYS:
        v = B.extras["episode"][key]
        assert v.dim() == 0 and v.is_cuda and math.isfinite(float(v)) and (key == "outcome_steps" or 0.0 <= float(v) <= 1.0)
    assert int(B._outcome_accum.abs().sum()) == 0 and int(B._extras_ticket[0]) == 0 and float(B._extras_accum.abs().sum()) == 0.0
    with pytest.raises(RuntimeError, match="never switched on"):
        A.outcome_totals()
    # switching off returns to the plain launch and the plain extras; the totals stay
    B.enable_outcome_stats(False)
    assert B._outcome is None and set(B.extras["episode"]) == PLAIN_KEYS and B.outcome_totals() == totals
    if path == "step":
        for k in range(3):
            step_a(), step_b()
            assert_same(A, B, 100 + k)
        assert B.outcome_totals() == totals


# ----------------------------------------------------------------------------- the runner
@pytest.mark.parametrize("outcome_stats", [True, False])
def test_runner_logs_the_outcome_columns_only_when_switched_on(tmp_path, monkeypatch, outcome_stats):
    """Two iterations per agent at 64 envs on the captured device rollout.  A runner trains ONE agent per evolution (the predator in
    evolution 0), and an agent's ``progress.csv`` exists once it has trained, so "both agents' tables" takes two evolutions: one of two
    iterations for each agent.  With the statistics on, both tables have the five ``Episode/outcome_*`` columns with finite values; with
    them off they have none."""
    from legged_games_gym_amd.envs import a1_game, task_registry
    a1_game.register_dec()
    try:
        ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
        if outcome_stats:
            task_registry.get_cfgs("dec_high_level_game")[0].env.outcome_stats = True      # an attribute the env reads with getattr(), on this registration only
        env, runner = dec_runner(task_registry, tmp_path, monkeypatch, ckpt, 64)
        assert runner.device_path and (env._outcome is not None) == outcome_stats
        runner.learn(max_num_evolutions=2, num_learning_iterations=2, init_at_random_ep_len=True)
        torch.cuda.synchronize()
        for agent in ("pred", "prey"):
            assert runner.runners[agent]._game_rollout
            rows = list(csv.DictReader(open(os.path.join(runner.log_dir, agent, "progress.csv"))))
            assert len(rows) == 2
            cols = [c for c in rows[0] if c.startswith("Episode/outcome_")]
            assert {"Episode/rew_pred_pursuit", "Episode/rew_prey_evasion"} <= set(rows[0])
            if not outcome_stats:
                assert cols == [] and set(env.extras["episode"]) == PLAIN_KEYS
                continue
            assert sorted(cols) == sorted(f"Episode/{k}" for k in KEYS)
            for row in rows:
                for c in cols:
                    assert math.isfinite(float(row[c])), (agent, c, row[c])
        if outcome_stats:
            totals = env.outcome_totals()
            assert totals["episodes"] > 0 and totals["steps"] >= totals["episodes"]
    finally:
        a1_game.unregister_dec()


# ----------------------------------------------------------------------------- play_outcomes and the cross-play
A_IT, B_IT = 1, 2          # checkpoints of the short run: after the predator's evolution, after the prey's


@pytest.fixture(scope="module")
def short_run(tmp_path_factory):
    """One short run of two evolutions of one iteration at 64 envs: ``model_1.pt`` (A) and ``model_2.pt`` (B, whose prey was trained one
    iteration further).  B's predator is then perturbed in the file, so that the two checkpoints' predators act differently."""
    from legged_games_gym_amd.envs import a1_game, task_registry
    root = tmp_path_factory.mktemp("dec_outcome_run")
    mp = pytest.MonkeyPatch()
    a1_game.register_dec()
    try:
        ckpt = write_ll_checkpoint(str(root / "ll" / "model_0.pt"), seed=3)
        env_cfg = task_registry.get_cfgs("dec_high_level_game")[0]
        env_cfg.env.capture_dist, env_cfg.env.episode_length_s = 3.0, 0.29     # on this registration only: 15-step games and a wide capture distance,
        env, runner = dec_runner(task_registry, root, mp, ckpt, 64)           # so that episodes END within the 30 / 40 steps of the evaluations below
        assert int(env.max_episode_length) == 15                               # ceil(0.29 s / 0.02 s)
        runner.learn(max_num_evolutions=2, num_learning_iterations=1, init_at_random_ep_len=True)
        torch.cuda.synchronize()
        run_dir = runner.log_dir
        path_b = os.path.join(run_dir, f"model_{B_IT}.pt")
        d = torch.load(path_b, map_location="cpu", weights_only=True)
        g = torch.Generator().manual_seed(5)
        for key, value in d["pred"]["model_state_dict"].items():
            if key.startswith("actor."):
                value.add_(0.05 * torch.randn(value.shape, generator=g))
        torch.save(d, path_b)
        del env, runner
        yield dict(run_dir=run_dir, load_run=os.path.basename(run_dir))
    finally:
        mp.undo()
        a1_game.unregister_dec()


def _cli(short_run, *extra):
    return ["--task", "dec_high_level_game", "--headless", "--sim_device", DEV, "--rl_device", DEV, "--load_run", short_run["load_run"], *extra]


def test_play_outcomes_reports_the_totals_of_its_rollout(short_run, capsys):
    """``play_outcomes`` in process on the one-iteration checkpoint, 30 steps at 16 envs: the JSON next to the checkpoint has the keys, and
    its counts are the env's totals.  ``play`` afterwards still builds its 50 envs: the registered config was not touched."""
    from legged_games_gym_amd.scripts import play_dec_game as pd
    args = pd._args(_cli(short_run, "--checkpoint", str(A_IT), "--num_envs", "16", "--steps", "30", "--outcomes"))
    assert args.steps == 30 and args.outcomes and args.num_envs == 16
    env, result, path = pd.play_outcomes(args, steps=args.steps)
    assert path == os.path.join(short_run["run_dir"], f"outcomes_{A_IT}.json") and os.path.isfile(path)
    data = json.load(open(path))
    assert data == json.loads(json.dumps(result))
    assert set(data) == {"totals", "rates", "mean_steps", "num_envs", "steps", "task", "iteration", "path"}
    assert tuple(data["totals"]) == ot.COUNTS and set(data["rates"]) == {f"{k}_rate" for k in ot.FLAGS}
    totals = env.outcome_totals()
    assert data["num_envs"] == env.num_envs == 16 and data["steps"] == 30 and data["iteration"] == A_IT and data["task"] == "dec_high_level_game"
    assert data["totals"] == totals and totals["episodes"] > 0
    assert data["path"] == "graphed policy step"                    # the registered actor triple has the shared actor launch
    rates = pd.dec_outcome_rates(totals)
    for k, v in rates.items():
        got = data["mean_steps"] if k == "mean_steps" else data["rates"][k]
        assert (got is None and math.isnan(v)) or got == v
    text = capsys.readouterr().out
    assert "not counted" in text and "captured" in text and "ll_timed_out" in text
    env2 = pd.play(pd._args(_cli(short_run)), steps=3)
    assert env2.num_envs == 50 and torch.isfinite(env2.obs_buf_prey).all()


def test_crossplay_swaps_weights_under_one_graph_and_restores_the_start_exactly(short_run):
    """Checkpoints A and B at 32 envs for 40 steps per cell.  The 2 x 2 tables; cell (A, A) of the run over [A, B] equals, integer for
    integer, cell (A, A) of a run over [A] alone and the totals of ``play_outcomes`` on A with the same envs, steps and seed.  In a run
    over [A, B, A] the LAST cell is (A, A) again, played after eight others on the same env and graph: it must equal the first, as every
    other repeated pairing must -- the start state is restored exactly and the weights under the graph are the loaded ones.  Finally the
    device actors after a swap act as the torch modules of the checkpoints they claim to hold, and the two predators act differently."""
    from legged_games_gym_amd.scripts import crossplay_dec_game as cp
    from legged_games_gym_amd.scripts import play_dec_game as pd
    common = ("--num_envs", "32", "--steps", "40")
    args = cp._args(_cli(short_run, *common, "--checkpoints", f"{A_IT},{B_IT}"))
    assert args.checkpoints == [A_IT, B_IT] and args.steps == 40
    ev, both, path = cp.crossplay(args, args.checkpoints, steps=args.steps)
    assert path == os.path.join(short_run["run_dir"], f"crossplay_{A_IT}_{B_IT}.json")
    data = json.load(open(path))
    assert data == json.loads(json.dumps(both)) and data["checkpoints"] == [A_IT, B_IT] and data["num_envs"] == 32 and data["steps"] == 40
    assert data["path"] == "graphed policy step" and (data["rows"], data["columns"]) == ("predator", "prey")
    for name in ("capture_rate", "timed_out_rate", "mean_steps", "totals"):
        assert len(data[name]) == 2 and all(len(row) == 2 for row in data[name]), name
    for i in range(2):
        for j in range(2):
            cell = data["totals"][i][j]
            assert tuple(cell) == ot.COUNTS and cell["episodes"] > 0
            assert data["capture_rate"][i][j] == cell["captured"] / cell["episodes"] and data["mean_steps"][i][j] == cell["steps"] / cell["episodes"]
            assert data["timed_out_rate"][i][j] == cell["timed_out"] / cell["episodes"]

    # the weights under the graph are the ones loaded: the device actors against the torch modules of the checkpoints
    files = {c: torch.load(os.path.join(short_run["run_dir"], f"model_{c}.pt"), map_location=DEV, weights_only=True) for c in (A_IT, B_IT)}
    module = lambda agent, c: (lambda m: (m.load_state_dict(files[c][agent]["model_state_dict"]), m)[1])(copy.deepcopy(ev.modules[agent]))
    gen = torch.Generator().manual_seed(3)
    obs = {"pred": (2.0 * torch.randn(32, 3, generator=gen)).to(DEV), "prey": (2.0 * torch.randn(32, 16, generator=gen)).to(DEV)}
    with torch.no_grad():
        want = {(a, c): module(a, c).act_inference(obs[a]).detach() for a in ("pred", "prey") for c in (A_IT, B_IT)}
    assert float((want["pred", A_IT] - want["pred", B_IT]).abs().max()) > 1e-2          # B's predator was perturbed
    for c_pred, c_prey in ((A_IT, B_IT), (B_IT, A_IT)):
        ev.load(files[c_pred]["pred"]["model_state_dict"], files[c_prey]["prey"]["model_state_dict"])
        for agent, c in (("pred", c_pred), ("prey", c_prey)):
            got = ev.fused[agent].act_inference(obs[agent]).clone()
            tol = 1e-4 * max(1.0, float(want[agent, c].abs().max()))
            assert float((got - want[agent, c]).abs().max()) < tol, (agent, c)
        assert float((ev.fused["pred"].act_inference(obs["pred"]) - want["pred", B_IT if c_pred == A_IT else A_IT]).abs().max()) > 1e-2
    del ev

    _, alone, _ = cp.crossplay(cp._args(_cli(short_run, *common, "--checkpoints", str(A_IT))), [A_IT], steps=40)
    assert alone["totals"][0][0] == both["totals"][0][0]
    _, played, _ = pd.play_outcomes(pd._args(_cli(short_run, *common, "--checkpoint", str(A_IT), "--outcomes")), steps=40)
    assert played["totals"] == both["totals"][0][0]
    _, again, _ = cp.crossplay(cp._args(_cli(short_run, *common, "--checkpoints", f"{A_IT},{B_IT},{A_IT}")), [A_IT, B_IT, A_IT], steps=40)
    t = again["totals"]
    assert t[2][2] == t[0][0] == t[0][2] == t[2][0] == both["totals"][0][0]
    assert t[0][1] == t[2][1] == both["totals"][0][1] and t[1][0] == t[1][2] == both["totals"][1][0] and t[1][1] == both["totals"][1][1]


@pytest.mark.parametrize("termination", of.TERMINATIONS)
def test_outcome_kernel_matches_the_twin_directly(termination):
    """k_dec_outcome against the NumPy twin itself, not through k_dec_post: one launch at 257 envs (two workgroups, the second nearly empty),
    every per-env array, the episode sums and the episode means under the comparison tests/test_gpu_dec_game.py holds lg_dec_game_post to."""
    from tests.dec_game_fixtures import check_call
    c = of.case(257, termination)
    s = c["s"]
    call = dict(p=c["p"], step=c["step"], command_pred=s["command_pred"], ll_rew=s["ll_rew"], ll_reset=s["ll_reset"], ll_time_out=c["ll_time_out"])
    L = Launcher(s, [call])
    L.launch(0, counter_on_device=True)
    check_call(c["p"], s, L.outputs(), c["info"], c["want"], extra_ulp=2)
    assert c["want"]["reset_buf"].any() and not c["want"]["reset_buf"].all()
