"""The opponent pool of ``dec_high_level_game`` on the device (include/legged_dec_game_pool.h, rl/opponent_pool.py): ``lg_dec_pool_act`` is,
per 32-env block, bit-identical to ``lg_dec_game_act`` launched with that block's member; a one-member pool is the plain launch; the
separate launches at wide precision 0; a captured graph follows ``push`` and ``assign`` without recapture; the runner's schedule and its
checkpoints."""
import os

import numpy as np
import pytest
import torch

from tests import dec_game_twin as dt
from tests.dec_game_fixtures import dec_registered  # noqa: F401
from tests.test_gpu_dec_game import (BIAS_PRED, BIAS_PREY, DEV, HIDDEN, STD_PRED, STD_PREY, agent_actor, dec_runner, fused_pair, make_dec, outputs_struct,
                                     pack_params)
from tests.test_gpu_game import write_ll_checkpoint

pytestmark = pytest.mark.gpu

# three members per role, each with its own std and output bias: the spread of STD_* / BIAS_* of tests/test_gpu_dec_game.py, so that every
# member puts clipped columns on both sides of their ranges
PREY_MEMBERS = ((3, STD_PREY, BIAS_PREY), (13, (1.0, 0.5, 0.8, 0.6), (-0.7, 0.7, -2.2, 0.3)), (23, (0.3, 1.2, 1.5, 0.4), (0.2, -0.1, 3.0, -0.5)))
PRED_MEMBERS = ((5, STD_PRED, BIAS_PRED), (15, (0.7, 1.3), (-1.5, 1.5)), (25, (1.6, 0.5), (0.3, -0.2)))
SEED_PREY, SEED_PRED = 4242 + 7919, 4242 + 7919 + 104729
PREY_KEYS = ("command", "ll_commands", "mean", "sample", "sigma", "log_prob", "obs_copy")
PRED_KEYS = ("command", "mean", "sample", "sigma", "log_prob", "obs_copy")


@pytest.fixture(scope="module")
def actors():
    """Three prey and three predator members, the low-level actor, and a three-member pool per role (built once for the module)."""
    from legged_games_gym_amd import capi
    from legged_games_gym_amd.rl import ActorCritic, FusedActor
    assert capi.load_library().lg_mlp_wide_set_precision(1) == 1
    prey = [FusedActor(agent_actor("prey", s, std, bias), DEV, seed=11) for s, std, bias in PREY_MEMBERS]
    pred = [FusedActor(agent_actor("pred", s, std, bias), DEV, seed=12) for s, std, bias in PRED_MEMBERS]
    torch.manual_seed(4)
    ll = FusedActor(ActorCritic(235, 235, 12, actor_hidden_dims=HIDDEN, critic_hidden_dims=HIDDEN).to(DEV), DEV, seed=1)
    pools = {"prey": capi.dec_pool_create([m.handle for m in prey], "prey"), "pred": capi.dec_pool_create([m.handle for m in pred], "pred")}
    yield {"prey": prey, "pred": pred, "ll": ll, "pools": pools}
    torch.cuda.synchronize()
    for pool in pools.values():
        capi.dec_pool_destroy(pool)


class Launch:
    """Inputs and output tensors of one actor launch on ``n`` envs; ``plain`` / ``pooled`` fill the outputs with a marker, launch, and return
    clones of everything the launch writes."""

    def __init__(self, actors, n, counter_on_device, heading=1):
        self.a, self.n = actors, n
        gen = torch.Generator().manual_seed(500 + n)
        self.prey_obs, self.pred_obs = (torch.randn(n, 16, generator=gen) * 3.0).to(DEV), (torch.randn(n, 3, generator=gen) * 3.0).to(DEV)
        self.ll_obs = (torch.randn(n, 235, generator=gen) * 1.5).to(DEV)
        self.P = pack_params(dt.params(num_envs=n, heading_command=heading))
        step_value = 77 + n
        self.counter = torch.tensor([step_value - 1], dtype=torch.int64, device=DEV)       # the kernels read counter + 1
        self.step, self.ctr = (-1, self.counter.data_ptr()) if counter_on_device else (step_value, None)
        f = lambda *s: torch.full(s, -9.0, device=DEV)
        self.t = {"prey": dict(command=f(n, 4), ll_commands=f(n, 4), mean=f(n, 4), sample=f(n, 4), sigma=f(n, 4), log_prob=f(n), obs_copy=f(n, 16)),
                  "pred": dict(command=f(n, 2), mean=f(n, 2), sample=f(n, 2), sigma=f(n, 2), log_prob=f(n), obs_copy=f(n, 3)), "ll_actions": f(n, 12)}

    def _arguments(self):
        from legged_games_gym_amd import capi
        y, p = self.t["prey"], self.t["pred"]
        for group in (y, p, {"a": self.t["ll_actions"]}):
            for v in group.values():
                v.fill_(-9.0)
        B = capi.dec_game_buffers({"command_prey": y["command"].data_ptr(), "command_pred": p["command"].data_ptr(), "ll_commands": y["ll_commands"].data_ptr()})
        outs = [outputs_struct(**{k: g[k] for k in ("sample", "sigma", "log_prob", "obs_copy")}) for g in (p, y)]
        return B, outs, torch.cuda.current_stream().cuda_stream

    def _results(self):
        torch.cuda.synchronize()
        return {"prey": {k: v.clone() for k, v in self.t["prey"].items()}, "pred": {k: v.clone() for k, v in self.t["pred"].items()},
                "ll_actions": self.t["ll_actions"].clone()}

    def plain(self, prey, pred, det_pred=False, det_prey=False):
        from legged_games_gym_amd import capi
        B, (out_pred, out_prey), stream = self._arguments()
        y, p = self.t["prey"], self.t["pred"]
        assert capi.dec_game_act(pred.handle, prey.handle, self.a["ll"].handle, self.P, B, self.pred_obs.data_ptr(), self.prey_obs.data_ptr(), self.ll_obs.data_ptr(),
                                 self.t["ll_actions"].data_ptr(), p["mean"].data_ptr(), y["mean"].data_ptr(), SEED_PRED, SEED_PREY, self.step, self.ctr,
                                 det_pred, det_prey, out_pred, out_prey, stream) == 0
        return self._results()

    def pooled(self, slots_pred, slots_prey, det_pred=False, det_prey=False, pools=None, handles=None):
        """``slots_*``: a device int32 table, or None for a role that is not pooled (it then runs on member 0's handle).  A pooled role gets a
        NULL handle: the entry point ignores it."""
        from legged_games_gym_amd import capi
        pools = pools or self.a["pools"]
        B, (out_pred, out_prey), stream = self._arguments()
        y, p = self.t["prey"], self.t["pred"]
        h_pred, h_prey = handles or (None if slots_pred is not None else self.a["pred"][0].handle, None if slots_prey is not None else self.a["prey"][0].handle)
        rc = capi.dec_pool_act(h_pred, h_prey, self.a["ll"].handle, pools["pred"] if slots_pred is not None else None,
                               slots_pred.data_ptr() if slots_pred is not None else None, pools["prey"] if slots_prey is not None else None,
                               slots_prey.data_ptr() if slots_prey is not None else None, self.P, B, self.pred_obs.data_ptr(), self.prey_obs.data_ptr(),
                               self.ll_obs.data_ptr(), self.t["ll_actions"].data_ptr(), p["mean"].data_ptr(), y["mean"].data_ptr(), SEED_PRED, SEED_PREY,
                               self.step, self.ctr, det_pred, det_prey, out_pred, out_prey, stream)
        assert rc == 0, rc
        return self._results()


def rows_by_block(per_member, key, slots, n):
    """Row e of member ``clamp(slots)[e // 32]``'s result: what the pooled launch must write for env e."""
    env_slot = torch.as_tensor(slots).clamp(0, len(per_member) - 1).long().repeat_interleave(32)[:n].to(DEV)
    return torch.stack([m[key] for m in per_member])[env_slot, torch.arange(n, device=DEV)]


def slot_tables(blocks):
    """All 0, all 2, round-robin, reversed, and one with values outside the pool (the kernel clamps them to 0 .. 2)."""
    b = torch.arange(blocks)
    return [torch.zeros(blocks, dtype=torch.int32), torch.full((blocks,), 2, dtype=torch.int32), (b % 3).int(), ((blocks - 1 - b) % 3).int(),
            torch.tensor([99, -5, 1, 7][:blocks], dtype=torch.int32)]


# ----------------------------------------------------------------------------- 1. per block bit-identical to the plain launch with the block's member
@pytest.mark.parametrize("role", ["prey", "pred", "both"])
@pytest.mark.parametrize("counter_on_device", [False, True])
@pytest.mark.parametrize("n", [1, 33, 100])          # one partial block; a second block with a single live lane; four blocks with a ragged tail
def test_pooled_launch_is_bit_identical_per_block_to_the_plain_launch_with_the_blocks_member(actors, n, counter_on_device, role):
    L = Launch(actors, n, counter_on_device)
    want = [L.plain(actors["prey"][s], actors["pred"][s]) for s in range(3)]          # member s of BOTH roles on all n envs: the roles are independent
    for s in range(3):
        assert torch.equal(want[s]["ll_actions"], want[0]["ll_actions"]) and float(want[s]["prey"]["command"].min()) > -9.0
        assert torch.equal(want[s]["prey"]["sigma"], torch.tensor(PREY_MEMBERS[s][1], device=DEV).expand(n, 4))
        assert torch.equal(want[s]["pred"]["sigma"], torch.tensor(PRED_MEMBERS[s][1], device=DEV).expand(n, 2))
    assert not torch.equal(want[0]["prey"]["mean"], want[1]["prey"]["mean"]) and not torch.equal(want[1]["pred"]["mean"], want[2]["pred"]["mean"])
    if n == 100:                                                                      # some commands clip and some do not, for every member
        for s in range(3):
            for who in ("prey", "pred"):
                clipped = want[s][who]["command"][:, :2] != want[s][who]["sample"][:, :2]
                assert bool(clipped.any()) and bool((~clipped).any()), (s, who)
    blocks = (n + 31) // 32
    tables = slot_tables(blocks)
    for i, table in enumerate(tables):
        slots_prey = table.to(DEV) if role in ("prey", "both") else None
        other = tables[(i + 2) % len(tables)]                                         # "both": a different table per role
        slots_pred = (other if role == "both" else table).to(DEV) if role in ("pred", "both") else None
        got = L.pooled(slots_pred, slots_prey)
        for who, keys, slots, cpu in (("prey", PREY_KEYS, slots_prey, table), ("pred", PRED_KEYS, slots_pred, other if role == "both" else table)):
            for key in keys:
                expect = rows_by_block([w[who] for w in want], key, cpu, n) if slots is not None else want[0][who][key]
                assert expect.shape == got[who][key].shape and torch.equal(got[who][key], expect), (i, who, key, cpu.tolist())
        assert torch.equal(got["ll_actions"], want[0]["ll_actions"]), i
        assert torch.equal(got["prey"]["ll_commands"], got["prey"]["command"]) and torch.equal(got["prey"]["obs_copy"], L.prey_obs)
        assert int(L.counter[0]) == 77 + n - 1
    if n == 100 and not counter_on_device:
        # deterministic on the pooled role: its command is the clipped mean of the block's member, the other role still samples
        from legged_games_gym_amd import capi
        table = tables[2]
        slots = table.to(DEV)
        got = L.pooled(slots if role != "prey" else None, slots if role != "pred" else None, det_pred=role != "prey", det_prey=role != "pred")
        det = {"prey": rows_by_block([w["prey"] for w in want], "mean", table, n) if role != "pred" else want[0]["prey"]["sample"].clone(),
               "pred": rows_by_block([w["pred"] for w in want], "mean", table, n) if role != "prey" else want[0]["pred"]["sample"].clone()}
        scratch = torch.empty(n, 4, device=DEV)
        capi.dec_game_pre(L.P, capi.dec_game_buffers({"command_prey": det["prey"].data_ptr(), "command_pred": det["pred"].data_ptr(), "ll_commands": scratch.data_ptr()}),
                          torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(got["prey"]["command"], det["prey"]) and torch.equal(got["pred"]["command"], det["pred"]) and torch.equal(got["prey"]["ll_commands"], scratch)


def test_pooled_launch_matches_float64_forwards_of_each_blocks_member(actors):
    """k_pool_act against references computed outside any kernel, at the smallest size with a second block (n = 33, block 0 -> member 1,
    block 1 -> member 2 for the prey; 2 and 0 for the predator): each row's mean is the float64 forward (``actor_forward64`` from the
    modules' arrays) of its block's member, the low-level actions that of the low-level actor, within 1e-4 of the output scale, the bar
    of the split-bf16 actors (tests/test_gpu_dec_game.py)."""
    from tests.recurrent_ref import actor_forward64, actor_params64
    n = 33
    L = Launch(actors, n, False)
    slots = {"prey": torch.tensor([1, 2], dtype=torch.int32), "pred": torch.tensor([2, 0], dtype=torch.int32)}
    got = L.pooled(slots["pred"].to(DEV), slots["prey"].to(DEV))
    checks = [("low-level actions", got["ll_actions"], actor_forward64(*actor_params64(actors["ll"].ac.actor), L.ll_obs.cpu().double().numpy()))]
    for who, obs in (("prey", L.prey_obs), ("pred", L.pred_obs)):
        per_member = [actor_forward64(*actor_params64(m.ac.actor), obs.cpu().double().numpy()) for m in actors[who]]
        rows = slots[who].long().repeat_interleave(32)[:n].numpy()
        checks.append((f"{who} mean", got[who]["mean"], np.stack(per_member)[rows, np.arange(n)]))
    for name, have, want in checks:
        err, scale = float(np.abs(have.cpu().double().numpy() - want).max()), max(1.0, float(np.abs(want).max()))
        print(f"[observed] k_pool_act n {n} {name}: err {err:.3e}, scale {scale:.3f}")
        assert err < 1e-4 * scale, (name, err, scale)


def test_pool_creation_checks_every_members_shape_and_the_launch_the_pools_role(actors):
    from legged_games_gym_amd import capi
    info = capi.dec_pool_query(actors["pools"]["prey"])
    assert (info.count, info.role, info.device) == (3, 1, 0) and info.table
    assert capi.dec_pool_query(actors["pools"]["pred"]).role == 2
    with pytest.raises(RuntimeError, match=r"\(-4\)"):
        capi.dec_pool_create([actors["prey"][0].handle, actors["pred"][0].handle], "prey")      # the SECOND member has the wrong shape
    with pytest.raises(RuntimeError, match=r"\(-4\)"):
        capi.dec_pool_create([actors["ll"].handle], "pred")
    L = Launch(actors, 33, False)
    slots = torch.zeros(2, dtype=torch.int32, device=DEV)
    swapped = {"prey": actors["pools"]["pred"], "pred": actors["pools"]["prey"]}
    B, (out_pred, out_prey), stream = L._arguments()
    rc = capi.dec_pool_act(actors["pred"][0].handle, None, actors["ll"].handle, None, None, swapped["prey"], slots.data_ptr(), L.P, B, L.pred_obs.data_ptr(),
                           L.prey_obs.data_ptr(), L.ll_obs.data_ptr(), L.t["ll_actions"].data_ptr(), L.t["pred"]["mean"].data_ptr(), L.t["prey"]["mean"].data_ptr(),
                           SEED_PRED, SEED_PREY, 5, None, False, False, out_pred, out_prey, stream)
    torch.cuda.synchronize()
    assert rc == -4 and float(L.t["prey"]["command"].max()) == -9.0                  # a predator pool in the prey role: refused, nothing launched


# ----------------------------------------------------------------------------- 2. a one-member pool is the plain launch
@pytest.mark.parametrize("n", [2000, 4096])          # the registered size; more workgroups per role (128) than a third of the CUs
def test_one_member_pool_equals_the_plain_launch(actors, n):
    from legged_games_gym_amd import capi
    L = Launch(actors, n, True, heading=0)
    want = L.plain(actors["prey"][1], actors["pred"][2])
    pools = {"prey": capi.dec_pool_create([actors["prey"][1].handle], "prey"), "pred": capi.dec_pool_create([actors["pred"][2].handle], "pred")}
    try:
        blocks = (n + 31) // 32
        zeros = torch.zeros(blocks, dtype=torch.int32, device=DEV)
        stale = (torch.arange(blocks, dtype=torch.int32) - 3).to(DEV)              # a table written for a larger pool: every slot clamps to member 0
        for slots_pred, slots_prey in ((zeros, zeros), (stale, zeros), (zeros, stale)):
            got = L.pooled(slots_pred, slots_prey, pools=pools)
            for who, keys in (("prey", PREY_KEYS), ("pred", PRED_KEYS)):
                for key in keys:
                    assert torch.equal(got[who][key], want[who][key]), (who, key)
            assert torch.equal(got["ll_actions"], want["ll_actions"])
    finally:
        torch.cuda.synchronize()
        for pool in pools.values():
            capi.dec_pool_destroy(pool)


# ----------------------------------------------------------------------------- 3. the env: separate launches at wide precision 0
def prey_pool(live, capacity=2, num_envs=64, **kw):
    from legged_games_gym_amd.rl import OpponentPool
    return OpponentPool(live, lambda: agent_actor("prey", 0), capacity, "prey", seed=5, num_envs=num_envs, **kw)


def member_state(k):
    seed, std, bias = PREY_MEMBERS[k]
    return agent_actor("prey", seed, std, bias).state_dict()


def test_precision_0_takes_the_separate_launches_selected_by_block(tmp_path):
    from legged_games_gym_amd import capi
    from legged_games_gym_amd.rl import FusedActor
    lib = capi.load_library()
    n = 64
    env = make_dec(write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3), n, seed=9)
    env.reset()
    pred = FusedActor(agent_actor("pred", 6, STD_PRED, BIAS_PRED), DEV, seed=21 + 104729)
    live = FusedActor(agent_actor("prey", 8, STD_PREY, BIAS_PREY), DEV, seed=21)
    pool = prey_pool(live)
    assert pool.push(member_state(1)) == 1 and pool.filled == 1
    pool.set_slots([1, 0])
    gen = torch.Generator().manual_seed(3)
    obs_prey, obs_pred = (torch.randn(n, 16, generator=gen) * 3.0).to(DEV), (torch.randn(n, 3, generator=gen) * 3.0).to(DEV)
    sigma, log_prob = torch.empty(n, 4, device=DEV), torch.empty(n, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    old = lib.lg_mlp_wide_set_precision(0)
    try:
        (cp, mp), (cy, my), _, _ = env._act(pred, pool, obs_pred, obs_prey, obs_pred, obs_prey, False, False, out_prey={"sigma": sigma, "log_prob": log_prob})
        assert env.last_act_rc == -4
        torch.cuda.synchronize()
        cy, my, cp, mp = cy.clone(), my.clone(), cp.clone(), mp.clone()
        rows = []
        for member in pool.members[:2]:                                           # per member: lg_policy_act on all envs, the role's seed, this step
            a, mu = torch.empty(n, 4, device=DEV), torch.empty(n, 4, device=DEV)
            assert lib.lg_policy_act(member.handle, obs_prey.data_ptr(), a.data_ptr(), mu.data_ptr(), n, live.seed, 1, None, 0, stream) == 0
            rows.append((a, mu, member.ac.std.detach().expand(n, 4)))
        first = (torch.arange(n, device=DEV) < 32).unsqueeze(1)                   # block 0 -> member 1, block 1 -> member 0 (the live one)
        sample, mean, std = (torch.where(first, rows[1][k], rows[0][k]) for k in range(3))
        a_p, mu_p = torch.empty(n, 2, device=DEV), torch.empty(n, 2, device=DEV)
        assert lib.lg_policy_act(pred.handle, obs_pred.data_ptr(), a_p.data_ptr(), mu_p.data_ptr(), n, pred.seed, 1, None, 0, stream) == 0
        command, command_p, scratch = sample.clone(), a_p.clone(), torch.empty(n, 4, device=DEV)
        capi.dec_game_pre(env._P, capi.dec_game_buffers({"command_prey": command.data_ptr(), "command_pred": command_p.data_ptr(), "ll_commands": scratch.data_ptr()}), stream)
        torch.cuda.synchronize()
        assert torch.equal(cy, command) and torch.equal(my, mean) and torch.equal(cp, command_p) and torch.equal(mp, mu_p)
        assert not torch.equal(rows[0][1][:32], rows[1][1][:32]) and torch.equal(sigma, std)
        assert torch.equal(log_prob, torch.distributions.Normal(mean, std).log_prob(sample).sum(-1))
        assert live._host_step == 1 and pred._host_step == 1 and pool.members[1]._host_step == 0      # one step of the live actors' noise streams
    finally:
        lib.lg_mlp_wide_set_precision(old)
    # back at precision 1 the same call is the pooled launch
    env._act(pred, pool, obs_pred, obs_prey, obs_pred, obs_prey, False, False)
    torch.cuda.synchronize()
    assert env.last_act_rc == 0 and live._host_step == 2
    with pytest.raises(RuntimeError, match="sync_device"):                        # a re-created member would leave the pool's table dangling: refused on the host
        live.sync()
        pool.handle


# ----------------------------------------------------------------------------- 4. under a captured graph
def test_captured_graph_follows_push_and_assign_without_recapture(tmp_path):
    """A: ``make_graphed_policy_step(pred, pool)`` on the prey role.  Every replay is checked per block against eager ``step_policy`` calls on a
    second env B that is given the observations and the noise step A's replay read, with the block's member as the prey: the actor stage depends
    on nothing else.  Between the two replays member 1 is OVERWRITTEN in place (the ring wraps) and the slot table is re-assigned."""
    from legged_games_gym_amd.rl import FusedActor
    n = 64
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    A, B = make_dec(ckpt, n, seed=9), make_dec(ckpt, n, seed=9)
    for env in (A, B):
        torch.manual_seed(90)
        env.reset()
    pred, live = fused_pair(A)
    pool = prey_pool(live)
    pool.push(member_state(1))
    slots = pool.assign(torch.Generator().manual_seed(1))
    assert sorted(slots.tolist()) == [0, 1]                                       # two blocks, share 0.5: one live, one snapshot
    replay = A.make_graphed_policy_step(pred, pool, warmup=3)
    assert A.last_act_rc == 0
    # host-counting twins over the SAME torch modules: B's eager launches (refreshed with sync_device after a push)
    pred_b = FusedActor(pred.ac, DEV, seed=pred.seed)
    twins = [FusedActor(m.ac, DEV, seed=live.seed) for m in pool.members]

    def check(expected_slots):
        obs_prey, obs_pred = A.obs_buf_prey.clone(), A.obs_buf_pred.clone()
        counter = int(A.ll_env._sim.buf["step_counter"][0])
        replay()
        torch.cuda.synchronize()
        got_y, got_my = (t.clone() for t in live.output_buffers(n))
        got_p, got_mp = (t.clone() for t in pred.output_buffers(n))
        assert int(A.ll_env._sim.buf["step_counter"][0]) == counter + 1 and torch.isfinite(A.obs_buf_prey).all()
        per_member = {}
        for s in sorted(set(expected_slots)):
            B.obs_buf_prey.copy_(obs_prey); B.obs_buf_pred.copy_(obs_pred)
            pred_b._host_step = twins[s]._host_step = counter                    # the replay's kernels read counter + 1
            (cp, mp), (cy, my), _ = B.step_policy(pred_b, twins[s])
            torch.cuda.synchronize()
            assert B.last_act_rc == 0
            per_member[s] = (cy.clone(), my.clone())
            assert torch.equal(got_p, cp) and torch.equal(got_mp, mp), s          # the predator side: unchanged by the prey's pool
        for b, s in enumerate(expected_slots):
            rows = slice(32 * b, 32 * b + 32)
            assert torch.equal(got_y[rows], per_member[s][0][rows]) and torch.equal(got_my[rows], per_member[s][1][rows]), (b, s)
        return got_my

    mean_1 = check(slots.tolist())
    pool.push(member_state(2))                                                    # -> member 2
    pool.push(member_state(0))                                                    # -> member 1, overwritten in place underneath the graph
    assert pool.filled == 2
    for twin in twins[1:]:
        twin.sync_device()
    pool.latest_share = 0.0                                                       # both blocks meet snapshots
    slots = pool.assign(torch.Generator().manual_seed(2))
    assert sorted(slots.tolist()) == [1, 2]
    mean_2 = check(slots.tolist())
    assert not torch.equal(mean_1, mean_2)


# ----------------------------------------------------------------------------- 5. the runner
def test_runner_pushes_at_the_start_of_an_evolution_and_checkpoints_the_pools(tmp_path, monkeypatch, dec_registered):
    from legged_games_gym_amd.utils.helpers import get_load_path
    reg = dec_registered
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    keys = dict(opponent_pool_size=2, opponent_latest_share=0.5, num_steps_per_env=8)
    env, runner = dec_runner(reg, tmp_path, monkeypatch, ckpt, 64, **keys)
    assert runner.device_path and set(runner.pools) == {"pred", "prey"}
    assert runner.views["pred"].opponent is runner.pools["prey"] and runner.views["prey"].opponent is runner.pools["pred"]
    assert runner.pools["pred"].live is runner.runners["pred"]._fused and runner.pools["pred"].capacity == 2
    state = lambda a: {k: v.detach().clone() for k, v in runner.runners[a].alg.actor_critic.state_dict().items()}
    same = lambda x, y: set(x) == set(y) and all(torch.equal(x[k], y[k]) for k in x)
    pred_0 = state("pred")
    runner.learn(max_num_evolutions=1, num_learning_iterations=1, init_at_random_ep_len=True)
    pred_1 = state("pred")
    assert not same(pred_0, pred_1) and runner.pools["pred"].filled == 1 and runner.pools["prey"].filled == 0
    assert same(runner.pools["pred"].members[1].ac.state_dict(), pred_0)          # pushed at the START of evolution 0: strictly earlier than the live member
    runner.learn(max_num_evolutions=2, num_learning_iterations=1)
    torch.cuda.synchronize()
    assert runner.current_evolution == 3 and runner.pools["pred"].filled == 2 and runner.pools["prey"].filled == 1
    assert same(runner.pools["pred"].members[2].ac.state_dict(), pred_1) and not same(state("pred"), pred_1)
    log_dir = str(tmp_path / "logs" / "dec_high_level_game")
    path = get_load_path(log_dir)
    assert path.endswith("model_3.pt")
    end_of_0 = torch.load(os.path.join(os.path.dirname(path), "model_1.pt"), map_location=DEV, weights_only=True)
    assert same(runner.pools["pred"].members[2].ac.state_dict(), end_of_0["pred"]["model_state_dict"])      # ... as saved at the end of evolution 0
    d = torch.load(path, map_location=DEV, weights_only=True)
    assert set(d) == {"pred", "prey", "evolution", "iter", "pool"} and set(d["pool"]) == {"pred", "prey"}
    assert d["pool"]["pred"]["filled"] == 2 and d["pool"]["prey"]["filled"] == 1 and len(d["pool"]["pred"]["snapshots"]) == 2
    rows = open(os.path.join(os.path.dirname(path), "progress.csv")).read().strip().splitlines()
    assert [r.split(",")[2] for r in rows[1:]] == ["pred", "prey", "pred"]
    assert torch.isfinite(env.obs_buf_prey).all() and torch.isfinite(env.rew_buf_pred).all()
    # the assignment before evolution 2 (prey pool, one snapshot, two blocks): one live block, one snapshot block
    assert sorted(runner.pools["prey"]._slots_host.tolist()) == [0, 1] and torch.equal(runner.pools["prey"]._slots.cpu(), runner.pools["prey"]._slots_host)
    # a fresh runner restores the pools
    _, fresh = dec_runner(reg, tmp_path, monkeypatch, ckpt, 64, log=False, **keys)
    assert fresh.pools["pred"].filled == 0
    fresh.load(path)
    torch.cuda.synchronize()
    assert fresh.current_evolution == 3
    for a in ("pred", "prey"):
        assert fresh.pools[a].filled == runner.pools[a].filled and fresh.pools[a]._next == runner.pools[a]._next
        for mine, theirs, saved in zip(fresh.pools[a].members[1:], runner.pools[a].members[1:], d["pool"][a]["snapshots"]):
            assert same(mine.ac.state_dict(), saved) and same(mine.ac.state_dict(), theirs.ac.state_dict())
        obs = getattr(env, f"obs_buf_{a}")                                          # ... and their device actors follow
        for k in (1, 2):
            assert torch.equal(fresh.pools[a].members[k].act_inference(obs), runner.pools[a].members[k].act_inference(obs))
    # the generic path has no pooled launch
    with pytest.raises(ValueError, match="device_rollout"):
        dec_runner(reg, tmp_path, monkeypatch, ckpt, 64, device_rollout=False, log=False, **keys)
