"""-m gpu: the outcome statistics per pool member of the decentralised game -- ``lg_dec_member_outcome_post`` (include/
legged_dec_game_member_outcome.h) writes what ``lg_dec_outcome_post`` writes, bit for bit, and keeps per pool member exactly the counts of the
NumPy twin (tests/dec_member_outcome_twin.py); the totals carried over consecutive launches and graph replays under a slot table rewritten in
place; every step path of the env with a pool bound; the runner's ``opponents.csv``, its prioritised deal and its checkpoints.  Nothing here
reads outside the tree."""
import csv
import os

import numpy as np
import pytest
import torch

from tests import dec_game_twin as dt
from tests import dec_member_outcome_fixtures as mf
from tests import dec_member_outcome_twin as mt
from tests import dec_outcome_fixtures as of
from tests import dec_outcome_twin as ot
from tests.dec_game_fixtures import dec_registered  # noqa: F401
from tests.test_gpu_dec_game import STATE, agent_actor, dec_runner, fused_pair, make_dec
from tests.test_gpu_dec_outcome import PER_ENV, Launcher, arrange, int_view, torch_policies
from tests.test_gpu_game import write_ll_checkpoint

pytestmark = pytest.mark.gpu
F = np.float32
DEV = "cuda:0"


# ----------------------------------------------------------------------------- the kernel without an env
class MemberLauncher(Launcher):
    """``Launcher`` of tests/test_gpu_dec_outcome.py with the buffers of ``lg_dec_member_outcome_buffers``: ONE slot table (rewritten in place
    by ``set_slots``) and one pair of member accumulators / totals for all calls."""

    def __init__(self, state, calls, slots, count):
        from legged_games_gym_amd import capi
        super().__init__(state, calls)
        blocks = (self.n + mt.BLOCK - 1) // mt.BLOCK
        self.slots = torch.zeros(blocks, dtype=torch.int32, device=DEV)
        self.maccum = torch.zeros(mt.ROWS, 6, dtype=torch.int64, device=DEV)
        self.mtotals = torch.zeros(mt.ROWS, 6, dtype=torch.int64, device=DEV)
        self.M = capi.dec_member_outcome_buffers({"block_slot": self.slots.data_ptr(), "member_accum": self.maccum.data_ptr(), "member_totals": self.mtotals.data_ptr()}, count)
        self.set_slots(slots)

    def set_slots(self, slots):
        slots = torch.from_numpy(np.ascontiguousarray(slots, np.int32))
        assert slots.shape == self.slots.shape
        self.slots.copy_(slots)

    def launch(self, k, counter_on_device):
        from legged_games_gym_amd import capi
        d = self.per_call[k]
        capi.dec_member_outcome_post(d["P"], d["B"], d["O"], self.M, -1 if counter_on_device else self.calls[k]["step"], torch.cuda.current_stream().cuda_stream)

    def member_stats(self):
        """-> (member_accum, member_totals) (synchronises)."""
        torch.cuda.synchronize()
        return self.maccum.cpu().numpy(), self.mtotals.cpu().numpy()


def call_of(c):
    s = c["s"]
    return dict(p=c["p"], step=c["step"], command_pred=s["command_pred"], ll_rew=s["ll_rew"], ll_reset=s["ll_reset"], ll_time_out=c["ll_time_out"])


@pytest.mark.parametrize("n", mf.SIZES)
def test_one_launch_is_bit_identical_to_the_pooled_one_and_counts_per_member_exactly(n):
    """One launch of ``lg_dec_outcome_post`` and, per slot table, one of ``lg_dec_member_outcome_post`` on the same inputs.  Bit-identical: every
    per-env array, the five pooled means, the pooled totals, both pooled accumulators and the ticket back at zero.  ``episode_means`` is a float
    sum that the workgroups add with atomics: bit-identical where its order is fixed -- up to two workgroups, ``a + b = b + a`` -- and at 2000
    envs (eight workgroups, where two launches of EITHER kernel may differ in the last bits) within ``dec_game_twin.means_bound`` of the twin,
    the bound tests/test_gpu_dec_outcome.py holds ``lg_dec_outcome_post`` itself to.  Per member: ``member_totals`` equals the twin exactly, its
    column sums are the pooled totals, ``member_accum`` is zero.  At 1 env no env is done: ``member_totals`` stays as it was (a marker)."""
    c = mf.case(n)
    odd = bool(n % 2)
    ref = Launcher(c["s"], [call_of(c)])
    ref.launch(0, counter_on_device=odd)
    want, (w_accum, w_extras, w_ticket, w_means, w_totals) = ref.outputs(), ref.stats()
    np.testing.assert_array_equal(w_totals, c["counts"])
    if n >= 64:
        members, double = mf.coverage(n)
        assert all(v >= 2 for v in members.values()) and double >= 1, (members, double)          # the pass below cannot be empty
    for name, table, count in mf.slot_tables(n):
        L = MemberLauncher(c["s"], [call_of(c)], table, count)
        marker = np.arange(mt.ROWS * 6, dtype=np.int64).reshape(mt.ROWS, 6) + 7
        L.mtotals.copy_(torch.from_numpy(marker))
        L.launch(0, counter_on_device=odd)
        got = L.outputs()
        for k in PER_ENV:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
            np.testing.assert_array_equal(int_view(got[k]), int_view(want[k]), err_msg=f"{name}: {k}")
        if n <= 512:
            np.testing.assert_array_equal(got["episode_means"].view(np.uint32), want["episode_means"].view(np.uint32), err_msg=name)
        else:
            bound = dt.means_bound(c["p"], c["info"])
            dm = np.abs(got["episode_means"].astype(np.float64) - c["want"]["episode_means"].astype(np.float64))
            print(f"n {n} {name}: episode means off the twin by {dm.tolist()}, bound {bound.tolist()}")
            assert (dm <= bound).all(), (dm, bound)
        accum, extras_accum, ticket, means, totals = L.stats()
        np.testing.assert_array_equal(means.view(np.uint32), w_means.view(np.uint32), err_msg=name)
        np.testing.assert_array_equal(totals, w_totals, err_msg=name)
        assert not accum.any() and not extras_accum.any() and ticket == 0 and not w_accum.any() and not w_extras.any() and w_ticket == 0
        maccum, mtotals = L.member_stats()
        rows = mf.member_counts(n, name)
        print(f"n {n} {name} count {count}: members {np.nonzero(rows[:, 0])[0].tolist()} episodes {rows[:, 0][rows[:, 0] > 0].tolist()}")
        np.testing.assert_array_equal(mtotals - marker, rows, err_msg=name)
        np.testing.assert_array_equal((mtotals - marker).sum(axis=0), totals, err_msg=name)
        assert not maccum.any(), name
        assert np.array_equal(L.slots.cpu().numpy(), table)                                        # the table is read, not written
        if int(c["counts"][0]) == 0:
            assert n == 1 and np.array_equal(mtotals, marker)
    assert n == 1 or int(c["counts"][0]) > 0


def test_member_totals_carried_over_three_launches_and_follow_a_rewritten_table_under_a_graph():
    """Three consecutive launches at 257 envs on one set of buffers (the third without a done env), the twin fed the state the device left:
    ``member_totals`` adds up call by call, the quiet call leaves it as it was, ``member_accum`` reads zero after every call.  Then the same
    three launches captured into ONE graph and replayed from the restored inputs, first under the table of the capture, then under another
    table written in place into the same buffer: the counts follow the new table without recapture and the totals accumulate."""
    p, state0, calls = of.sequence_inputs()
    calls = calls[:3]
    assert of.SEQ_QUIET == 2
    n, blocks = of.SEQ_N, (of.SEQ_N + 31) // 32
    table_a, table_b, count = (np.arange(blocks) % 4).astype(np.int32), ((np.arange(blocks) * 3 + 1) % 7 - 1).astype(np.int32), 6      # b holds -1: clamped
    L = MemberLauncher(state0, calls, table_a, count)
    running, per_call = np.zeros((mt.ROWS, 6), np.int64), []
    for k, c in enumerate(calls):
        before = L.state()
        s = dict(before, env_origins=state0["env_origins"], command_pred=c["command_pred"], ll_rew=c["ll_rew"], ll_reset=c["ll_reset"])
        _, info = dt.post(c["p"], s, step=c["step"])
        f = ot.flags(info, c["ll_reset"], c["ll_time_out"])
        per_call.append((f, before["curr_episode_step"].copy()))
        rows = mt.member_counts(f, before["curr_episode_step"], table_a, count)
        L.launch(k, counter_on_device=bool(k % 2))
        maccum, mtotals = L.member_stats()
        if k == of.SEQ_QUIET:
            assert not rows.any() and np.array_equal(mtotals, running)
        else:
            assert int(rows[:, 0].sum()) > 0
        running = running + rows
        np.testing.assert_array_equal(mtotals, running, err_msg=f"call {k}")
        assert not maccum.any() and not L.stats()[0].any() and L.stats()[2] == 0, k
        np.testing.assert_array_equal(mtotals.sum(axis=0), L.stats()[4])
    assert (running[:4, 0] > 0).all() and not running[4:].any()
    pooled = L.stats()[4].copy()

    want_b = sum(mt.member_counts(f, step, table_b, count) for f, step in per_call)
    assert not np.array_equal(want_b, running) and np.array_equal(want_b.sum(axis=0), running.sum(axis=0))
    L.restore(state0)
    L.totals.zero_(); L.means.zero_(); L.mtotals.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for k in range(len(calls)):
            L.launch(k, counter_on_device=bool(k % 2))
    expect = np.zeros_like(running)
    for rep, (table, rows) in enumerate(((table_a, running), (table_b, want_b), (table_a, running))):
        L.restore(state0)
        L.set_slots(table)                                                       # in place: the graph holds the buffer's address
        graph.replay()
        maccum, mtotals = L.member_stats()
        expect = expect + rows
        np.testing.assert_array_equal(mtotals, expect, err_msg=f"replay {rep}")
        assert not maccum.any()
        np.testing.assert_array_equal(L.stats()[4], (rep + 1) * pooled)


# ----------------------------------------------------------------------------- the env, every path
def prey_pool(live, num_envs):
    """A pool on the prey role, capacity 2, with 2 pushes."""
    from legged_games_gym_amd.rl import OpponentPool
    pool = OpponentPool(live, lambda: agent_actor("prey", 0), 2, "prey", seed=5, num_envs=num_envs)
    assert pool.push(agent_actor("prey", 13, (1.0, 0.5, 0.8, 0.6), (-0.7, 0.7, -2.2, 0.3)).state_dict(), pushed_at=4) == 1
    assert pool.push(agent_actor("prey", 23, (0.3, 1.2, 1.5, 0.4), (0.2, -0.1, 3.0, -0.5)).state_dict()) == 2
    assert pool.filled == 2 and pool.pushed_at == [4, None]
    blocks = (num_envs + 31) // 32
    pool.set_slots([2, 1] if blocks == 2 else [b % 3 for b in range(blocks)])
    return pool


def assert_same(A, B, k):
    for name in STATE:
        assert torch.equal(getattr(A, name), getattr(B, name)), (k, name)
    for name in ("root_states", "dof_state", "obs_buf", "commands"):
        assert torch.equal(getattr(A.ll_env, name), getattr(B.ll_env, name)), (k, name)
    assert torch.equal(A._outcome_means, B._outcome_means) and torch.equal(A._outcome_totals, B._outcome_totals), k


@pytest.mark.parametrize("n", [64, 300])
@pytest.mark.parametrize("path", ["step", "graphed_step", "step_policy", "graphed_policy_step"])
def test_env_paths_are_unchanged_by_binding_a_pool_and_the_members_add_up(tmp_path, path, n):
    """24 steps on one step path of two identically seeded envs with the outcome statistics on, B with a pool bound as well: the state, the
    pooled means and the pooled totals bit-equal at every step; B's per-member counts summed over the members equal ``outcome_totals()``, and
    the episodes per member equal the done envs of the member's blocks summed over the steps."""
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    A, B = make_dec(ckpt, n, seed=9), make_dec(ckpt, n, seed=9)
    for env in (A, B):
        env.enable_outcome_stats()
        env.capture_dist = 2.5
        env.set_command_ranges()
        torch.manual_seed(90)
        env.reset()
    graphed = path.startswith("graphed")
    (pa, ya), (pb, yb) = fused_pair(A if path == "graphed_policy_step" else None), fused_pair(B if path == "graphed_policy_step" else None)
    pool_a, pool_b = prey_pool(ya, n), prey_pool(yb, n)
    B.enable_member_outcomes(pool_b)                                             # before a capture: the graph keeps the launch the switch selected
    assert B._member_outcome.count == 3 and A._member_outcome is None
    if path in ("step", "graphed_step"):
        pol_p, pol_y = torch_policies()
        if path == "step":
            step_a, step_b = (lambda: A.step(pol_p(A.obs_buf_pred), pol_y(A.obs_buf_prey))), (lambda: B.step(pol_p(B.obs_buf_pred), pol_y(B.obs_buf_prey)))
        else:
            step_a, step_b = A.make_graphed_step(pol_p, pol_y, warmup=3), B.make_graphed_step(pol_p, pol_y, warmup=3)
    elif path == "step_policy":
        step_a, step_b = (lambda: A.step_policy(pa, pool_a)), (lambda: B.step_policy(pb, pool_b))
    else:
        step_a, step_b = A.make_graphed_policy_step(pa, pool_a, warmup=3), B.make_graphed_policy_step(pb, pool_b, warmup=3)
    for env in (A, B):
        arrange(env)
        env.reset_outcome_totals()                                               # (the reset and the warm-up steps of a capture were counted too)
    pool_b.reset_member_totals()
    assert_same(A, B, -1)
    member = torch.from_numpy(mt.env_member(pool_b._slots_host.numpy(), n, 3)).to(DEV)
    episodes = torch.zeros(3, dtype=torch.int64, device=DEV)
    for k in range(24):
        step_a(), step_b()
        assert_same(A, B, k)
        episodes += torch.bincount(member[B.reset_buf], minlength=3)
    torch.cuda.synchronize()
    if path.endswith("policy_step") or path == "step_policy":
        assert A.last_act_rc == 0 and B.last_act_rc == 0
    totals, rows = B.outcome_totals(), pool_b.member_totals_host()
    print(f"{path} n {n}: {totals}; per member {[r['episodes'] for r in rows]}")
    assert A.outcome_totals() == totals and totals["episodes"] >= 16 and len(rows) == 3
    assert {k: sum(r[k] for r in rows) for k in ot.COUNTS} == totals
    assert [r["episodes"] for r in rows] == episodes.tolist()
    assert sum(r["episodes"] > 0 for r in rows) >= 2
    assert not pool_b.member_totals[3:].any() and not pool_b.member_accum.any() and not pool_a.member_totals.any()
    assert int(B._outcome_accum.abs().sum()) == 0 and int(B._extras_ticket[0]) == 0
    if not graphed:
        # unbinding returns to lg_dec_outcome_post: the pooled totals go on, the members' stay
        B.enable_member_outcomes(None)
        for k in range(3):
            step_a(), step_b()
            assert_same(A, B, 100 + k)
        assert pool_b.member_totals_host() == rows


def test_push_zeroes_row_0_and_the_overwritten_row_only_and_binding_needs_the_statistics(tmp_path):
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    env = make_dec(ckpt, 64, seed=9)
    _, live = fused_pair()
    pool = prey_pool(live, 64)
    with pytest.raises(RuntimeError, match="enable_outcome_stats"):
        env.enable_member_outcomes(pool)
    assert env._member_outcome is None
    env.enable_outcome_stats()
    env.enable_member_outcomes(pool)
    assert env._member_outcome.count == 3 and env._member_pool is pool
    env.enable_member_outcomes(None)
    assert env._member_outcome is None and env._member_pool is None
    marker = torch.arange(1, 16 * 6 + 1, dtype=torch.int64).reshape(16, 6)
    pool.member_totals.copy_(marker)
    address = pool.member_totals.data_ptr()
    assert pool.member_totals_host()[2] == dict(zip(ot.COUNTS, marker[2].tolist())) and len(pool.member_totals_host()) == 3
    assert pool.push(agent_actor("prey", 3).state_dict(), pushed_at=9) == 1      # the ring wraps: member 1 is overwritten
    want = marker.clone()
    want[0], want[1] = 0, 0
    assert torch.equal(pool.member_totals.cpu(), want) and pool.member_totals.data_ptr() == address and pool.pushed_at == [9, None]
    pool.reset_member_totals(rows=[5])
    want[5] = 0
    assert torch.equal(pool.member_totals.cpu(), want)
    state = pool.state()
    assert state["pushed_at"] == [9, -1] and torch.equal(state["member_totals"], want) and state["member_totals"].device.type == "cpu"
    pool.reset_member_totals()
    assert not pool.member_totals.any() and pool.member_totals.data_ptr() == address
    pool.pushed_at = [None, None]
    pool.load_state(state)
    assert pool.pushed_at == [9, None] and torch.equal(pool.member_totals.cpu(), want) and pool.member_totals.data_ptr() == address


# ----------------------------------------------------------------------------- the runner
def read_rows(log_dir):
    rows = list(csv.DictReader(open(os.path.join(log_dir, "opponents.csv"))))
    assert list(rows[0]) == ["evolution", "agent", "member", "pushed_at", "blocks", "episodes", "captured", "timed_out", "fell", "ll_timed_out", "steps", "learner_win_rate"]
    return rows


def runner_with_pool(reg, tmp_path, monkeypatch, **keys):
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    env_cfg = reg.get_cfgs("dec_high_level_game")[0]
    env_cfg.env.outcome_stats = True                                            # an attribute the env reads with getattr(), on this registration only
    env_cfg.env.capture_dist, env_cfg.env.episode_length_s = 3.0, 0.29          # 15-step games and a wide capture distance: episodes END within the short rollouts
    keys = dict(dict(opponent_pool_size=2, num_steps_per_env=8), **keys)
    env, runner = dec_runner(reg, tmp_path, monkeypatch, ckpt, 64, **keys)
    assert runner.device_path and env._outcome is not None and set(runner.pools) == {"pred", "prey"}
    return ckpt, keys, env, runner


def filled_before(evolution, agent):
    """Snapshots in ``agent`` 's pool when evolution ``evolution`` deals: one push per earlier-or-equal evolution that trained ``agent``."""
    return min(2, sum(1 for e in range(evolution + 1) if ("pred", "prey")[e % 2] == agent))


def test_runner_logs_the_members_and_keeps_the_uniform_deal_at_priority_0_and_checkpoints_the_counts(tmp_path, monkeypatch, dec_registered):
    from legged_games_gym_amd.rl.opponent_pool import assign_blocks, learner_win_rate
    reg = dec_registered
    ckpt, keys, env, runner = runner_with_pool(reg, tmp_path, monkeypatch, opponent_latest_share=0.5)
    assert runner.priority == 0.0
    env.reset_outcome_totals()
    seen = dict.fromkeys(ot.COUNTS, 0)
    for e in range(4):
        agent, other = ("pred", "prey")[e % 2], ("prey", "pred")[e % 2]
        before = env.outcome_totals()
        runner.learn(max_num_evolutions=1, num_learning_iterations=2, init_at_random_ep_len=(e == 0))
        torch.cuda.synchronize()
        pool, filled = runner.pools[other], filled_before(e - 1, other) if e else 0
        assert pool.filled == filled and env._member_pool is pool
        want = assign_blocks(2, filled, 0.5, torch.Generator().manual_seed((runner.seed * 1000003 + e) & 0x7FFFFFFFFFFFFFFF))      # the parent's seed rule
        assert torch.equal(pool._slots_host, want) and torch.equal(pool._slots.cpu(), want), e
        rows = [r for r in read_rows(runner.log_dir) if int(r["evolution"]) == e]
        assert [int(r["member"]) for r in rows] == list(range(filled + 1)) and all(r["agent"] == agent for r in rows)
        assert [int(r["blocks"]) for r in rows] == torch.bincount(want.long(), minlength=filled + 1).tolist() and sum(int(r["blocks"]) for r in rows) == 2
        assert [r["pushed_at"] for r in rows] == [""] + [str(p) for p in pool.pushed_at[:filled]]
        now = env.outcome_totals()
        for k in ot.COUNTS:                                                     # every launch of the evolution was counted for exactly one member
            assert sum(int(r[k]) for r in rows) == now[k] - before[k], (e, k)
            seen[k] += sum(int(r[k]) for r in rows)
        for r in rows:
            rate = learner_win_rate({k: int(r[k]) for k in ot.COUNTS}, agent)
            assert (r["learner_win_rate"] == "" and int(r["episodes"]) == 0) or float(r["learner_win_rate"]) == rate
            assert int(r["episodes"]) > 0 or int(r["blocks"]) == 0
        assert now["episodes"] > before["episodes"]
    assert seen == env.outcome_totals() and runner.current_evolution == 4
    assert runner.pools["pred"].pushed_at == [0, 2] and runner.pools["prey"].pushed_at == [1, 3]
    # the push at the start of evolution 3 zeroed row 0 and row 2 of the prey's pool; row 1 keeps what evolution 2 counted
    prey_rows = runner.pools["prey"].member_totals_host()
    assert prey_rows[0]["episodes"] == 0 and prey_rows[2]["episodes"] == 0
    assert prey_rows[1] == {k: int(r[k]) for r in read_rows(runner.log_dir) if (r["evolution"], r["member"]) == ("2", "1") for k in ot.COUNTS}

    # checkpoints: the keys, a fresh runner, and a checkpoint written without the new keys
    path = os.path.join(runner.log_dir, f"model_{runner.current_learning_iteration}.pt")
    d = torch.load(path, map_location=DEV, weights_only=True)
    assert set(d) == {"pred", "prey", "evolution", "iter", "pool"}
    assert set(d["pool"]["pred"]) == {"filled", "next", "snapshots", "pushed_at", "member_totals"} and d["pool"]["pred"]["pushed_at"] == [0, 2]
    _, fresh = dec_runner(reg, tmp_path, monkeypatch, ckpt, 64, log=False, **keys)
    assert fresh.pools["pred"].pushed_at == [None, None] and not fresh.pools["pred"].member_totals.any()
    fresh.load(path)
    torch.cuda.synchronize()
    for a in ("pred", "prey"):
        assert fresh.pools[a].pushed_at == runner.pools[a].pushed_at and fresh.pools[a].filled == runner.pools[a].filled
        assert torch.equal(fresh.pools[a].member_totals, runner.pools[a].member_totals) and fresh.pools[a].member_totals_host() == runner.pools[a].member_totals_host()
    assert int(runner.pools["pred"].member_totals.sum()) > 0
    for a in ("pred", "prey"):
        del d["pool"][a]["pushed_at"], d["pool"][a]["member_totals"]
    old = str(tmp_path / "old_format.pt")
    torch.save(d, old)
    _, fresh = dec_runner(reg, tmp_path, monkeypatch, ckpt, 64, log=False, **keys)
    fresh.load(old)
    torch.cuda.synchronize()
    assert fresh.current_evolution == 4
    for a in ("pred", "prey"):
        assert fresh.pools[a].filled == 2 and fresh.pools[a].pushed_at == [None, None] and not fresh.pools[a].member_totals.any()


def test_runner_deals_by_priority_from_the_logged_counts(tmp_path, monkeypatch, dec_registered):
    """``opponent_priority`` 1 with no live block (share 0), so that both 32-env blocks are dealt over the snapshots.  Before every evolution
    the weights the runner computes and the deal it then makes are recomputed here from ``opponents.csv`` alone: the running counts of a
    snapshot are the sums of its rows of the earlier evolutions of the same learner (same member, same ``pushed_at``)."""
    from legged_games_gym_amd.rl.opponent_pool import apportion, pfsp_weights
    reg = dec_registered
    _, _, env, runner = runner_with_pool(reg, tmp_path, monkeypatch, opponent_latest_share=0.0, opponent_priority=1.0)
    assert runner.priority == 1.0
    met = 0
    for e in range(4):
        agent, other = ("pred", "prey")[e % 2], ("prey", "pred")[e % 2]
        runner.learn(max_num_evolutions=1, num_learning_iterations=2, init_at_random_ep_len=(e == 0))
        torch.cuda.synchronize()
        pool = runner.pools[other]
        filled = pool.filled
        assert filled == (filled_before(e - 1, other) if e else 0)
        rows = read_rows(runner.log_dir)
        wins, episodes = [], []
        for m in range(1, filled + 1):
            mine = [r for r in rows if int(r["evolution"]) < e and r["agent"] == agent and int(r["member"]) == m and r["pushed_at"] == str(pool.pushed_at[m - 1])]
            n, captured = sum(int(r["episodes"]) for r in mine), sum(int(r["captured"]) for r in mine)
            episodes.append(n)
            wins.append(captured if agent == "pred" else n - captured)
        met += sum(n > 0 for n in episodes)
        weights = pfsp_weights(wins, episodes, 1.0)
        counts = torch.bincount(pool._slots_host.long(), minlength=filled + 1).tolist()
        print(f"evolution {e} ({agent}): wins {wins} of {episodes}, weights {weights}, blocks {counts}")
        if filled == 0:
            assert counts == [2]
            continue
        assert counts == [0] + apportion(weights, 2) and all(c >= 1 for c in counts[1:])      # every filled member keeps a block
        assert [int(r["blocks"]) for r in rows if int(r["evolution"]) == e] == counts
    assert met >= 1                                                              # evolution 3 dealt with counts of evolution 1 on the table
    # the weights the runner would compute NOW for the next evolution (the predator's, against the prey's pool), from the csv as well
    rows = read_rows(runner.log_dir)
    pool = runner.pools["prey"]
    wins, episodes = [], []
    for m in (1, 2):
        mine = [r for r in rows if r["agent"] == "pred" and int(r["member"]) == m and r["pushed_at"] == str(pool.pushed_at[m - 1])]
        episodes.append(sum(int(r["episodes"]) for r in mine))
        wins.append(sum(int(r["captured"]) for r in mine))
    assert runner.opponent_weights("pred") == pfsp_weights(wins, episodes, 1.0) and episodes[0] > 0 and episodes[1] == 0


@pytest.mark.parametrize("n", [33, 300])
def test_member_kernel_matches_the_twin_directly(n):
    """k_member_outcome against the NumPy twin itself, not through k_dec_outcome: one launch under the cycling slot table at 33 envs (a wave
    that holds two members) and at 300 (a second workgroup with a ragged last block), every per-env array, the episode sums and the episode
    means under the comparison tests/test_gpu_dec_game.py holds lg_dec_game_post to."""
    from tests.dec_game_fixtures import check_call
    c = mf.case(n)
    name, table, count = next(t for t in mf.slot_tables(n) if t[0] == "cycle")
    L = MemberLauncher(c["s"], [call_of(c)], table, count)
    L.launch(0, counter_on_device=bool(n % 2))
    check_call(c["p"], c["s"], L.outputs(), c["info"], c["want"], extra_ulp=2)
    assert c["want"]["reset_buf"].any() and not c["want"]["reset_buf"].all()
