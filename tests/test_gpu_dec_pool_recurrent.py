"""-m gpu: the opponent pool for recurrent policies of ``dec_high_level_game`` (include/legged_dec_pool_recurrent.h, rl.RecurrentOpponentPool).
``lg_dec_pool_lstm_step`` / ``lg_dec_pool_lstm_act`` are, per 32-env block, bit-identical to ``lg_dec_lstm_step`` / ``lg_dec_game_lstm_act`` launched
with the block's member as the role's handle; both hold the float64 bars of the plain launches; a captured graph follows ``push`` and
``set_slots`` without recapture; the env's pooled launches equal its separate launches; the runner's schedule, ``opponents.csv`` and checkpoints;
cross-play of recurrent checkpoints.  Nothing here reads outside the tree."""
import csv
import math
import os

import numpy as np
import pytest
import torch

from tests import dec_game_twin as dt
from tests.recurrent_ref import actor_forward64, actor_params64, lstm_params64, lstm_step64
from tests.test_gpu_dec_game import assert_same_state, make_dec, pack_params
from tests.test_gpu_dec_game_recurrent import TOL, _dec_runner, _guarded, _ll, _recurrent_policy, _same_memories, _stream
from tests.test_gpu_dec_member_outcome import filled_before
from tests.test_gpu_dec_pool import PRED_MEMBERS, PREY_MEMBERS, rows_by_block, slot_tables
from tests.test_gpu_game import write_ll_checkpoint
from tests.dec_game_fixtures import dec_registered  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED_PRED, SEED_PREY = 4242 + 104729, 4242
SIZES = [1, 33, 65]          # one partial block; a second block of one row; a third block
# (predator units, predator hidden widths, prey units, prey hidden widths): 32 and 256 units in the same cell launch (1 and 8 waves, the
# narrower role's surplus waves idle), the 32-32-32 actor next to the default 512-256-128 with its 136 KB of LDS -- each role on each shape
SHAPES = {"pred32_prey256": (32, (32, 32, 32), 256, (512, 256, 128)), "pred256_prey32": (256, (512, 256, 128), 32, (32, 32, 32))}
ROLE_IN = {"pred": 3, "prey": 16}
ACTIONS = {"pred": 2, "prey": 4}
_cache = {}


def _module(agent, units, hidden, seed, std, bias):
    ac = _recurrent_policy(agent, units=units, hidden=hidden, seed=seed)
    with torch.no_grad():
        ac.std.copy_(torch.tensor(std))
        ac.actor[-1].bias.copy_(torch.tensor(bias))
    return ac


def _members(shape):
    """Three ``RecurrentFusedActor`` s per role with different weights, stds and last biases, and an ``lg_dec_rpool`` per role over them."""
    from legged_games_gym_amd import capi
    from legged_games_gym_amd.rl.recurrent_actor import RecurrentFusedActor
    if shape not in _cache:
        up, hp, uy, hy = SHAPES[shape]
        pred = [RecurrentFusedActor(_module("pred", up, hp, s, std, bias), DEV, seed=12) for s, std, bias in PRED_MEMBERS]
        prey = [RecurrentFusedActor(_module("prey", uy, hy, s, std, bias), DEV, seed=11) for s, std, bias in PREY_MEMBERS]
        pools = {who: capi.dec_rpool_create([m.lstm_a.handle for m in ms], [m.fused.handle for m in ms], who) for who, ms in (("pred", pred), ("prey", prey))}
        _cache[shape] = {"pred": pred, "prey": prey, "pools": pools, "units": {"pred": up, "prey": uy}}
    return _cache[shape]


def _pool_args(M, slots_pred, slots_prey):
    return (M["pools"]["pred"] if slots_pred is not None else None, slots_pred.data_ptr() if slots_pred is not None else None,
            M["pools"]["prey"] if slots_prey is not None else None, slots_prey.data_ptr() if slots_prey is not None else None)


def _tables_for(role, tables, i):
    """(CPU table of the predator or None, of the prey or None): with "both" a different table per role."""
    table, other = tables[i], tables[(i + 2) % len(tables)]
    return (other if role == "both" else table) if role in ("pred", "both") else None, table if role in ("prey", "both") else None


# ----------------------------------------------------------------------------- 1. the cell launch
ROLES = ("pred", "pred", "prey", "prey")     # predator actor / critic memory, prey actor / critic memory


def _cell_inputs(shape, n):
    M = _members(shape)
    gen = torch.Generator().manual_seed(3000 + n)
    reset = torch.zeros(n + 5, dtype=torch.uint8)
    reset[:n] = (torch.arange(n) % 3 == 1).to(torch.uint8)
    reset[n:] = 1
    reset = reset.to(DEV)
    x = {who: _guarded(n, ROLE_IN[who], torch.rand(n, ROLE_IN[who], generator=gen) * 6.0 - 3.0) for who in ("pred", "prey")}
    h, c = [], []
    for who in ROLES:
        for dst in (h, c):
            t = _guarded(n, M["units"][who], torch.rand(n, M["units"][who], generator=gen) * 2.0 - 1.0)
            t[:n][reset[:n] != 0] = float("nan")                                   # a reset row's stale state is not read
            dst.append(t)
    return M, x, h, c, reset


def _cell_roles(M, member, x, h, c, outs, pooled=(False, False)):
    """The four roles with ``member`` in the two actor-memory roles (a NULL handle where the role is pooled) and member 0's critic memories."""
    handles = (None if pooled[0] else M["pred"][member].lstm_a.handle, M["pred"][0].lstm_c.handle,
               None if pooled[1] else M["prey"][member].lstm_a.handle, M["prey"][0].lstm_c.handle)
    return [(handles[r], x[ROLES[r]].data_ptr(), h[r].data_ptr(), c[r].data_ptr(), outs[r][0].data_ptr(), outs[r][1].data_ptr()) for r in range(4)]


def _cell_plain(M, member, x, h, c, reset, n):
    from legged_games_gym_amd import capi
    outs = [(_guarded(n, M["units"][who]), _guarded(n, M["units"][who])) for who in ROLES]
    capi.dec_lstm_step(_cell_roles(M, member, x, h, c, outs), reset.data_ptr(), n, _stream())
    torch.cuda.synchronize()
    return outs


def _cell_pooled(M, x, h, c, reset, n, slots_pred, slots_prey):
    from legged_games_gym_amd import capi
    outs = [(_guarded(n, M["units"][who]), _guarded(n, M["units"][who])) for who in ROLES]
    capi.dec_pool_lstm_step(_cell_roles(M, 0, x, h, c, outs, (slots_pred is not None, slots_prey is not None)), *_pool_args(M, slots_pred, slots_prey),
                            reset.data_ptr(), n, _stream())
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("role", ["prey", "pred", "both"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_pooled_cell_launch_is_bit_identical_per_block_to_the_plain_launch_with_the_blocks_member(shape, n, role):
    M, x, h, c, reset = _cell_inputs(shape, n)
    want = [_cell_plain(M, s, x, h, c, reset, n) for s in range(3)]                # member s in BOTH actor-memory roles on all n envs
    for r in (0, 2):
        assert bool(torch.isfinite(want[0][r][0][:n]).all()) and not torch.equal(want[0][r][0][:n], want[1][r][0][:n])
    for r in (1, 3):                                                               # the critic memories are member 0's in every launch
        assert torch.equal(want[1][r][0][:n], want[0][r][0][:n]) and torch.equal(want[2][r][1][:n], want[0][r][1][:n])
    tables = slot_tables((n + 31) // 32)
    for i in range(len(tables)):
        cpu_pred, cpu_prey = _tables_for(role, tables, i)
        got = _cell_pooled(M, x, h, c, reset, n, cpu_pred.to(DEV) if cpu_pred is not None else None, cpu_prey.to(DEV) if cpu_prey is not None else None)
        for r, cpu in ((0, cpu_pred), (1, None), (2, cpu_prey), (3, None)):
            for k, name in enumerate(("h", "c")):
                expect = rows_by_block([{"v": w[r][k][:n]} for w in want], "v", cpu, n) if cpu is not None else want[0][r][k][:n]
                assert torch.equal(got[r][k][:n], expect), (i, r, name, None if cpu is None else cpu.tolist())
                assert bool(torch.isnan(got[r][k][n:]).all()), (i, r, name, "guard rows written")


# ----------------------------------------------------------------------------- 2. the actor launch
KEYS = {"prey": ("command", "ll_commands", "mean", "sample", "sigma", "log_prob", "obs_copy"), "pred": ("command", "mean", "sample", "sigma", "log_prob", "obs_copy")}


class ActorLaunch:
    """Inputs and outputs of one actor launch on ``n`` envs (NaN guard rows behind row n of every tensor)."""

    def __init__(self, shape, n, heading=1):
        self.M, self.n = _members(shape), n
        gen = torch.Generator().manual_seed(700 + n)
        u = self.M["units"]
        self.h = {who: _guarded(n, u[who], torch.rand(n, u[who], generator=gen) * 2.0 - 1.0) for who in ("pred", "prey")}
        self.obs = {who: _guarded(n, ROLE_IN[who], torch.randn(n, ROLE_IN[who], generator=gen) * 3.0) for who in ("pred", "prey")}
        self.ll_obs = _guarded(n, 235, torch.randn(n, 235, generator=gen) * 1.5)
        self.P = pack_params(dt.params(num_envs=n, heading_command=heading))
        self.step = 77 + n

    def _outputs(self):
        from legged_games_gym_amd import capi
        n = self.n
        t = {who: dict(command=_guarded(n, ACTIONS[who]), mean=_guarded(n, ACTIONS[who]), sample=_guarded(n, ACTIONS[who]), sigma=_guarded(n, ACTIONS[who]),
                       log_prob=_guarded(n, 0), obs_copy=_guarded(n, ROLE_IN[who])) for who in ("pred", "prey")}
        t["prey"]["ll_commands"] = _guarded(n, 4)
        t["ll_actions"] = _guarded(n, 12)
        B = capi.dec_game_buffers({"command_prey": t["prey"]["command"].data_ptr(), "command_pred": t["pred"]["command"].data_ptr(),
                                   "ll_commands": t["prey"]["ll_commands"].data_ptr()})
        outs = []
        for who in ("pred", "prey"):
            o = capi.lg_dec_act_outputs()
            for field in ("sample", "sigma", "log_prob", "obs_copy"):
                setattr(o, field, t[who][field].data_ptr())
            outs.append(o)
        return t, B, outs

    def _tail(self, t, B, outs, det_pred, det_prey):
        return (self.P, B, self.h["pred"].data_ptr(), self.h["prey"].data_ptr(), self.obs["pred"].data_ptr(), self.obs["prey"].data_ptr(), self.ll_obs.data_ptr(),
                t["ll_actions"].data_ptr(), t["pred"]["mean"].data_ptr(), t["prey"]["mean"].data_ptr(), SEED_PRED, SEED_PREY, self.step, None, det_pred, det_prey,
                outs[0], outs[1], _stream())

    def _results(self, t):
        torch.cuda.synchronize()
        n = self.n
        for who in ("pred", "prey"):
            for k, v in t[who].items():
                assert bool(torch.isnan(v[n:]).all()), f"{who} {k}: the guard rows behind row {n} were written"
        return {"pred": {k: v[:n] for k, v in t["pred"].items()}, "prey": {k: v[:n] for k, v in t["prey"].items()}, "ll_actions": t["ll_actions"][:n]}

    def plain(self, member, det_pred=False, det_prey=False):
        from legged_games_gym_amd import capi
        t, B, outs = self._outputs()
        assert capi.dec_game_lstm_act(self.M["pred"][member].fused.handle, self.M["prey"][member].fused.handle, _ll()[1].handle,
                                      *self._tail(t, B, outs, det_pred, det_prey)) == 0
        return self._results(t)

    def pooled(self, slots_pred, slots_prey, det_pred=False, det_prey=False):
        """A pooled role gets a NULL handle: the entry point ignores it.  A role without a table runs on member 0's handle."""
        from legged_games_gym_amd import capi
        t, B, outs = self._outputs()
        rc = capi.dec_pool_lstm_act(None if slots_pred is not None else self.M["pred"][0].fused.handle, None if slots_prey is not None else self.M["prey"][0].fused.handle,
                                    _ll()[1].handle, *_pool_args(self.M, slots_pred, slots_prey), *self._tail(t, B, outs, det_pred, det_prey))
        assert rc == 0, rc
        return self._results(t)


@pytest.mark.parametrize("deterministic", [False, True], ids=["sampled", "deterministic"])
@pytest.mark.parametrize("role", ["prey", "pred", "both"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_pooled_actor_launch_is_bit_identical_per_block_to_the_plain_launch_with_the_blocks_member(shape, n, role, deterministic):
    from legged_games_gym_amd import capi
    assert capi.load_library().lg_mlp_wide_set_precision(-1) == 1
    L = ActorLaunch(shape, n)
    det = dict(det_pred=deterministic, det_prey=deterministic)
    want = [L.plain(s, **det) for s in range(3)]
    for s in range(3):
        assert torch.equal(want[s]["ll_actions"], want[0]["ll_actions"])
        assert torch.equal(want[s]["prey"]["sigma"], torch.tensor(PREY_MEMBERS[s][1], device=DEV).expand(n, 4))
        assert torch.equal(want[s]["pred"]["sigma"], torch.tensor(PRED_MEMBERS[s][1], device=DEV).expand(n, 2))
        for who in ("pred", "prey"):
            assert torch.equal(want[s][who]["sample"], want[s][who]["mean"]) == deterministic, (s, who)
    assert not torch.equal(want[0]["prey"]["mean"], want[1]["prey"]["mean"]) and not torch.equal(want[1]["pred"]["mean"], want[2]["pred"]["mean"])
    tables = slot_tables((n + 31) // 32)
    for i in range(len(tables)):
        cpu_pred, cpu_prey = _tables_for(role, tables, i)
        got = L.pooled(cpu_pred.to(DEV) if cpu_pred is not None else None, cpu_prey.to(DEV) if cpu_prey is not None else None, **det)
        for who, cpu in (("prey", cpu_prey), ("pred", cpu_pred)):
            for key in KEYS[who]:
                expect = rows_by_block([w[who] for w in want], key, cpu, n) if cpu is not None else want[0][who][key]
                assert expect.shape == got[who][key].shape and torch.equal(got[who][key], expect), (i, who, key, None if cpu is None else cpu.tolist())
        assert torch.equal(got["ll_actions"], want[0]["ll_actions"]), i
        assert torch.equal(got["prey"]["ll_commands"], got["prey"]["command"]) and torch.equal(got["prey"]["obs_copy"], L.obs["prey"][:n])


def test_pool_query_and_refusals_on_real_handles():
    from legged_games_gym_amd import capi
    M = _members("pred32_prey256")
    info = capi.dec_rpool_query(M["pools"]["prey"])
    assert (info.count, info.role, info.device, info.num_in, info.hidden, info.ksteps) == (3, 1, 0, 16, 256, 136) and info.table
    assert list(info.dims) == [256, 512, 256, 128, 4] and info.max_width == 512
    info = capi.dec_rpool_query(M["pools"]["pred"])
    assert (info.count, info.role, info.num_in, info.hidden) == (3, 2, 3, 32) and list(info.dims) == [32, 32, 32, 32, 2]
    other = _members("pred256_prey32")
    with pytest.raises(RuntimeError, match=r"\(-4\)"):                                 # the SECOND member has another shape
        capi.dec_rpool_create([M["prey"][0].lstm_a.handle, other["prey"][0].lstm_a.handle], [M["prey"][0].fused.handle, other["prey"][0].fused.handle], "prey")
    with pytest.raises(RuntimeError, match=r"\(-4\)"):                                 # a predator as a prey
        capi.dec_rpool_create([M["pred"][0].lstm_a.handle], [M["pred"][0].fused.handle], "prey")
    L = ActorLaunch("pred32_prey256", 33)
    t, B, outs = L._outputs()
    slots = torch.zeros(2, dtype=torch.int32, device=DEV)
    rc = capi.dec_pool_lstm_act(M["pred"][0].fused.handle, None, _ll()[1].handle, None, None, M["pools"]["pred"], slots.data_ptr(), *L._tail(t, B, outs, False, False))
    torch.cuda.synchronize()
    assert rc == -4 and bool(torch.isnan(t["prey"]["command"]).all())                # a predator pool in the prey role: refused, nothing launched


# ----------------------------------------------------------------------------- 3. against float64 outside any kernel
def test_pooled_launches_match_float64_per_block_with_the_blocks_member():
    """n = 33: block 0 uses member 1 and block 1 member 2 (both roles).  The cell and the actors are restated per block in float64 with that
    member's weights; the bars are those tests/test_gpu_dec_game_recurrent.py holds the plain launches to (a block does the same
    arithmetic): ``TOL`` = 2e-5 of the scale for h and c, 2e-5 for the sampled roles' means, 1e-4 for the low-level actions (split bf16),
    2e-5 for the log-probs."""
    shape, n = "pred32_prey256", 33
    table = torch.tensor([1, 2], dtype=torch.int32)
    rows = table.long().repeat_interleave(32)[:n].numpy()
    M, x, h, c, reset = _cell_inputs(shape, n)
    slots = table.to(DEV)
    got = _cell_pooled(M, x, h, c, reset, n, slots, slots)
    flags = reset[:n].cpu().numpy()
    clean = lambda t: torch.nan_to_num(t[:n], nan=0.0).cpu().numpy()
    for r in range(4):
        who = ROLES[r]
        rnns = [(m.ac.memory_a if r in (0, 2) else M[who][0].ac.memory_c).rnn for m in M[who]]
        per_member = [lstm_step64(lstm_params64(rnn), x[who][:n].cpu().numpy(), clean(h[r]), clean(c[r]), flags) for rnn in rnns]
        for k, name in enumerate(("h", "c")):
            ref = np.stack([p[k] for p in per_member])[rows, np.arange(n)]
            err, scale = float(np.abs(got[r][k][:n].cpu().double().numpy() - ref).max()), max(1.0, float(np.abs(ref).max()))
            print(f"[observed] k_dec_pool_lstm_cell n {n} role {r} {name}: err {err:.3e}, scale {scale:.3f}, fraction of the bar {err / (TOL * scale):.3f}")
            assert err < TOL * scale, (r, name, err)
    L = ActorLaunch(shape, n)
    out = L.pooled(slots, slots)
    ll_want = actor_forward64(*actor_params64(_ll()[0].actor), L.ll_obs[:n].cpu().double().numpy())
    checks = [("low-level actions", out["ll_actions"], ll_want, 1e-4)]
    for who in ("pred", "prey"):
        per_member = [actor_forward64(*actor_params64(m.ac.actor), L.h[who][:n].cpu().double().numpy()) for m in M[who]]
        checks.append((f"{who} mean", out[who]["mean"], np.stack(per_member)[rows, np.arange(n)], 2e-5))
    for name, have, want, tol in checks:
        err, scale = float(np.abs(have.cpu().double().numpy() - want).max()), max(1.0, float(np.abs(want).max()))
        print(f"[observed] k_dec_pool_lstm_act n {n} {name}: err {err:.3e}, scale {scale:.3f}, fraction of the bar {err / (tol * scale):.3f}")
        assert err < tol * scale, (name, err, scale)
    for who in ("pred", "prey"):
        std = torch.stack([m.ac.std.detach().cpu().double() for m in M[who]])[torch.as_tensor(rows)]
        sample, mean = out[who]["sample"].cpu().double(), out[who]["mean"].cpu().double()
        assert torch.equal(out[who]["sigma"].cpu().double(), std)
        z = (sample - mean) / std
        want_lp = (-0.5 * z * z - std.log() - 0.5 * math.log(2.0 * math.pi)).sum(-1)
        err = float((out[who]["log_prob"].cpu().double() - want_lp).abs().max())
        print(f"[observed] k_dec_pool_lstm_act n {n} log_prob {who}: err {err:.3e}, max |z| {float(z.abs().max()):.2f}, fraction of the bar {err / 2e-5:.3f}")
        assert err < 2e-5, (who, err)


# ----------------------------------------------------------------------------- 4. under a captured graph
def _rec_pool(live, who, capacity=2, num_envs=None, units=64, hidden=(64, 64, 32)):
    from legged_games_gym_amd.rl import RecurrentOpponentPool
    return RecurrentOpponentPool(live, lambda: _recurrent_policy(who, units=units, hidden=hidden, seed=0), capacity, who, seed=5, num_envs=num_envs)


def test_captured_pooled_launches_follow_push_and_set_slots_without_recapture():
    """The two pooled launches captured once on a ``RecurrentOpponentPool`` of the prey.  ``push`` repacks a member in place and ``set_slots``
    rewrites the table in place (and zeroes the stale rows of the state the launches read): the next replay equals the eager launches."""
    from legged_games_gym_amd import capi
    from legged_games_gym_amd.rl.recurrent_actor import RecurrentFusedActor
    n = 65
    counter = torch.tensor([41], dtype=torch.int64, device=DEV)
    pred = RecurrentFusedActor(_recurrent_policy("pred"), DEV, seed=SEED_PRED, step_counter=counter, num_envs=n)
    live = RecurrentFusedActor(_recurrent_policy("prey"), DEV, seed=SEED_PREY, step_counter=counter, num_envs=n)
    pool = _rec_pool(live, "prey", num_envs=n)
    gen = torch.Generator().manual_seed(8)
    obs = {"pred": (torch.randn(n, 3, generator=gen) * 3.0).to(DEV), "prey": (torch.randn(n, 16, generator=gen) * 3.0).to(DEV)}
    ll_obs = (torch.randn(n, 235, generator=gen) * 1.5).to(DEV)
    for f in (pred, live):
        for t in f.state_a[0]:
            t.copy_(torch.rand(t.shape, generator=gen) * 2.0 - 1.0)
    reset = torch.zeros(n, dtype=torch.uint8, device=DEV)
    reset[5::7] = 1
    P = pack_params(dt.params(num_envs=n))

    def buffers():
        out = {k: torch.full((n, w), -9.0, device=DEV) for k, w in dict(command_pred=2, command_prey=4, ll_commands=4, ll_actions=12, mean_pred=2, mean_prey=4,
                                                                        h_pred=64, c_pred=64, h_prey=64, c_prey=64).items()}
        return out

    def launches(out):
        stream = _stream()
        roles = [(pred.lstm_a.handle, obs["pred"].data_ptr(), pred.state_a[0][0].data_ptr(), pred.state_a[0][1].data_ptr(), out["h_pred"].data_ptr(), out["c_pred"].data_ptr()),
                 None, (None, obs["prey"].data_ptr(), live.state_a[0][0].data_ptr(), live.state_a[0][1].data_ptr(), out["h_prey"].data_ptr(), out["c_prey"].data_ptr()), None]
        slots = pool.slot_table(n).data_ptr()
        capi.dec_pool_lstm_step(roles, None, None, pool.handle, slots, reset.data_ptr(), n, stream)
        B = capi.dec_game_buffers({k: out[k].data_ptr() for k in ("command_prey", "command_pred", "ll_commands")})
        assert capi.dec_pool_lstm_act(pred.fused.handle, None, _ll()[1].handle, None, None, pool.handle, slots, P, B, out["h_pred"].data_ptr(), out["h_prey"].data_ptr(),
                                      obs["pred"].data_ptr(), obs["prey"].data_ptr(), ll_obs.data_ptr(), out["ll_actions"].data_ptr(), out["mean_pred"].data_ptr(),
                                      out["mean_prey"].data_ptr(), SEED_PRED, SEED_PREY, -1, counter.data_ptr(), False, False, None, None, stream) == 0

    graphed, eager = buffers(), buffers()
    launches(eager)                                                                # the first call raises the LDS limits, outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launches(graphed)

    def check(tag):
        graph.replay()
        launches(eager)
        torch.cuda.synchronize()
        for k in graphed:
            assert not bool((graphed[k] == -9.0).any()), (tag, k, "not written")
            assert torch.equal(graphed[k], eager[k]), (tag, k)
        return {k: v.clone() for k, v in graphed.items()}

    first = check("all live")
    sd = {k: v + 0.05 for k, v in live.ac.state_dict().items()}
    assert pool.push(sd) == 1
    pool.set_slots([1, 0, 1])
    second = check("after push and set_slots")
    assert not torch.equal(first["mean_prey"][:32], second["mean_prey"][:32]) and not torch.equal(first["h_prey"][64:], second["h_prey"][64:])
    assert torch.equal(first["mean_pred"], second["mean_pred"]) and torch.equal(first["ll_actions"], second["ll_actions"])
    # the rows of the re-dealt blocks were zeroed in the state the launches read, block 1 (still live) kept its state
    assert float(live.state_a[0][0][:32].abs().max()) == 0.0 and float(live.state_a[0][0][64:].abs().max()) == 0.0 and float(live.state_a[0][0][32:64].abs().max()) > 0.0
    pool.push({k: v - 0.1 for k, v in live.ac.state_dict().items()})             # member 2
    counter.fill_(99)
    pool.set_slots([2, 2, 0])
    third = check("a second push, another table, another step")
    assert not torch.equal(third["mean_prey"], second["mean_prey"]) and not torch.equal(third["command_pred"], second["command_pred"])


# ----------------------------------------------------------------------------- 5. the env
N_ENV = 65


def _env_with_pool(ckpt, states):
    from legged_games_gym_amd.rl.recurrent_actor import RecurrentFusedActor
    env = make_dec(ckpt, N_ENV, seed=9)
    torch.manual_seed(90)
    env.reset()
    env.ll_env.episode_length_buf[::2] = int(env.ll_env.max_episode_length) - 2 - (torch.arange(0, N_ENV, 2, device=DEV) % 7)
    pred = RecurrentFusedActor(_recurrent_policy("pred"), DEV, seed=21 + 104729, num_envs=N_ENV)
    live = RecurrentFusedActor(_recurrent_policy("prey"), DEV, seed=21, num_envs=N_ENV)
    pool = _rec_pool(live, "prey", num_envs=N_ENV)
    for sd in states:
        pool.push(sd)
    return env, pred, live, pool


def test_env_pooled_launches_equal_the_separate_launches_and_a_redeal_zeroes_the_stale_blocks(tmp_path, capsys):
    """A: ``step_policy(RecurrentFusedActor, RecurrentOpponentPool)`` on the pooled launches.  B, identically seeded: the same env forced onto
    the separate launches (``step_memory_separate`` / ``act_separate``: one ``lg_lstm_step`` and one ``lg_lstm_actor_act`` per member in use, rows by
    block).  Four steps with forced resets and the learner's critic memory: commands, means, stored sample / sigma / log-prob, env state and
    both memories bit for bit.  Then a re-deal: the ``(h, c)`` rows of exactly the stale blocks are zero in both slots, the others untouched."""
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    base = _recurrent_policy("prey").state_dict()
    states = [{k: v + 0.05 for k, v in base.items()}, {k: v - 0.08 for k, v in base.items()}]
    A, pa, ya, pool_a = _env_with_pool(ckpt, states)
    B, pb, yb, pool_b = _env_with_pool(ckpt, states)
    B._recurrent_library = lambda fused, say=True, pooled=False: (B._say_separate("forced", say, pooled), (None, False))[1]
    for pool in (pool_a, pool_b):
        pool.set_slots([1, 2, 0])
    forced = torch.arange(3, N_ENV, 5, device=DEV)
    outs = [dict(sample=torch.empty(N_ENV, 2, device=DEV), sigma=torch.empty(N_ENV, 2, device=DEV), log_prob=torch.empty(N_ENV, device=DEV)) for _ in range(2)]
    capsys.readouterr()
    for k in range(4):
        res = [env.step_policy(p, pool, out_pred=o, with_critic_memory=("pred",)) for env, p, pool, o in ((A, pa, pool_a, outs[0]), (B, pb, pool_b, outs[1]))]
        torch.cuda.synchronize()
        assert A.last_act_rc == 0 and B.last_act_rc == -4, k
        (pred_a, prey_a, _), (pred_b, prey_b, _) = res
        for a, b, name in zip(pred_a + prey_a, pred_b + prey_b, ("command_pred", "mean_pred", "critic_pred", "command_prey", "mean_prey")):
            assert torch.equal(a, b), (k, name)
        for key in ("sample", "sigma", "log_prob"):
            print(f"[observed] step {k} stored {key}: max |pooled - separate| {float((outs[0][key] - outs[1][key]).abs().max()):.3e}")
            assert torch.equal(outs[0][key], outs[1][key]), (k, key)
        assert_same_state(A, B, k)
        assert _same_memories(pa, pb) and _same_memories(ya, yb), k
        assert pa._flip == pb._flip and ya._flip == yb._flip
        for env in (A, B):
            env.reset_buf[forced] = True
    said = capsys.readouterr().out
    lines = [line for line in said.splitlines() if line.startswith("[dec_high_level_game]")]      # one line, the first time
    assert len(lines) == 1 and "pooled recurrent actor launch unavailable (forced)" in lines[0] and "per member" in lines[0], said
    assert float(ya.hidden_states()[0][0].abs().max()) > 0.0
    # a re-deal: block 0 keeps member 1, block 1 changes (2 -> 0), block 2 keeps the live member; then member 1 is overwritten
    before = [[t.clone() for t in pair] for pair in ya.state_a]
    pool_a.set_slots([1, 0, 0])
    torch.cuda.synchronize()
    for pair, old in zip(ya.state_a, before):
        for t, o in zip(pair, old):
            assert float(t[32:64].abs().max()) == 0.0 and torch.equal(t[:32], o[:32]) and torch.equal(t[64:], o[64:])
    pool_a.push(states[1])                                                         # the ring's next member is 1: overwritten
    pool_a.set_slots([1, 0, 0])
    torch.cuda.synchronize()
    for pair, old in zip(ya.state_a, before):
        for t, o in zip(pair, old):
            assert float(t[:64].abs().max()) == 0.0 and torch.equal(t[64:], o[64:]) and float(o[64:].abs().max()) > 0.0


# ----------------------------------------------------------------------------- 6. the runner and cross-play
def _read_rows(log_dir):
    return list(csv.DictReader(open(os.path.join(log_dir, "opponents.csv"))))


def test_runner_trains_against_recurrent_pools_checkpoints_them_and_crossplay_resets_memories_per_cell(tmp_path, monkeypatch, dec_registered, capsys):
    from legged_games_gym_amd.rl import RecurrentOpponentPool
    from legged_games_gym_amd.scripts import crossplay_dec_game as cp
    from legged_games_gym_amd.scripts.play_dec_game import DecEvaluation
    reg = dec_registered
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    env_cfg, train_cfg = reg.get_cfgs("dec_high_level_game")
    saved = {k: getattr(env_cfg.env, k) for k in ("capture_dist", "episode_length_s")}
    try:
        env_cfg.env.outcome_stats = True                                           # an attribute the env reads with getattr(), on this registration only
        env_cfg.env.capture_dist, env_cfg.env.episode_length_s = 3.0, 0.29        # 15-step games and a wide capture distance: episodes END within the short rollouts
        keys = dict(opponent_pool_size=2, opponent_pool_recurrent=True, opponent_priority=1.0, num_steps_per_env=8, save_interval=2)
        env, runner, _ = _dec_runner(reg, tmp_path, monkeypatch, ckpt, n=64, **keys)
        assert runner.recurrent and runner.device_path and runner.pool_recurrent and env._outcome is not None
        assert all(isinstance(runner.pools[a], RecurrentOpponentPool) for a in ("pred", "prey"))
        assert runner.views["pred"].opponent is runner.pools["prey"] and runner.pools["prey"].live is runner.runners["prey"]._fused
        for e in range(4):
            agent, other = ("pred", "prey")[e % 2], ("prey", "pred")[e % 2]
            runner.learn(max_num_evolutions=1, num_learning_iterations=2, init_at_random_ep_len=(e == 0))
            torch.cuda.synchronize()
            pool = runner.pools[other]
            assert env._member_pool is pool and pool.filled == (filled_before(e - 1, other) if e else 0), (e, pool.filled)
            rows = [r for r in _read_rows(runner.log_dir) if int(r["evolution"]) == e]
            assert [int(r["member"]) for r in rows] == list(range(pool.filled + 1)) and all(r["agent"] == agent for r in rows)
            assert sum(int(r["blocks"]) for r in rows) == pool._slots_host.numel() == 2
            assert sum(int(r["episodes"]) for r in rows) > 0
        assert runner.pools["pred"].filled == 2 and runner.pools["prey"].filled == 2 and runner.current_evolution == 4
        assert runner.pools["pred"].pushed_at == [0, 2] and runner.pools["prey"].pushed_at == [1, 3]
        said = capsys.readouterr().out
        assert "unavailable" not in said, said
        assert all(bool(torch.isfinite(p).all()) for a in ("pred", "prey") for p in runner.runners[a].alg.actor_critic.parameters())

        # a checkpoint saved and loaded into a fresh runner reproduces the pools' snapshots and slots
        path = os.path.join(runner.log_dir, f"model_{runner.current_learning_iteration}.pt")
        d = torch.load(path, map_location=DEV, weights_only=True)
        assert set(d) == {"pred", "prey", "evolution", "iter", "pool"} and "memory_a.rnn.weight_hh_l0" in d["pool"]["prey"]["snapshots"][0]
        log_dir = runner.log_dir
        _, fresh, _ = _dec_runner(reg, tmp_path, monkeypatch, ckpt, n=64, **keys)
        fresh.load(path)
        torch.cuda.synchronize()
        for a in ("pred", "prey"):
            mine, theirs = fresh.pools[a], runner.pools[a]
            assert (mine.filled, mine._next, mine.pushed_at) == (theirs.filled, theirs._next, theirs.pushed_at)
            assert torch.equal(mine.member_totals, theirs.member_totals)
            for m, t in zip(mine.members[1:], theirs.members[1:]):
                assert all(torch.equal(x, y) for x, y in zip(m.ac.state_dict().values(), t.ac.state_dict().values()))
            assert torch.equal(mine._slots_host, theirs._slots_host) and torch.equal(mine._slots.cpu(), theirs._slots_host) and not mine._marked
        assert torch.equal(d["pool"]["pred"]["slots"].cpu(), runner.pools["pred"]._slots_host)
        for name in ("opponent_pool_size", "opponent_pool_recurrent", "opponent_priority"):       # the evaluation below builds two policies, no pools
            delattr(train_cfg.runner, name)

        # cross-play A, B, A: the two A rows / columns give identical cells, a diagonal cell equals a fresh evaluation of that checkpoint alone
        its = sorted(int(f[6:-3]) for f in os.listdir(log_dir) if f.startswith("model_") and f.endswith(".pt"))
        a_it, b_it = its[0], its[-1]
        assert a_it != b_it
        argv = ["--task", "dec_high_level_game", "--num_envs", "64", "--headless", "--sim_device", DEV, "--rl_device", DEV, "--policy_class_name", "ActorCriticRecurrent",
                "--rnn_hidden_size", "64", "--load_run", os.path.basename(log_dir)]
        args = cp._args(argv + ["--steps", "24", "--checkpoints", f"{a_it},{b_it},{a_it}"])
        ev, result, out = cp.crossplay(args, args.checkpoints, steps=args.steps)
        assert ev.recurrent and ev.path == "graphed policy step" and os.path.isfile(out)
        T = result["totals"]
        assert T[0] == T[2] and [row[0] for row in T] == [row[2] for row in T]
        assert sum(cell["episodes"] for row in T for cell in row) > 0
        from legged_games_gym_amd.scripts.play_dec_game import _args as play_args
        single = play_args(argv + ["--steps", "24"])
        single.checkpoint = b_it
        alone = DecEvaluation(single)
        assert alone.recurrent and alone.iteration == b_it
        assert {k: int(v) for k, v in alone.run(24).items()} == T[1][1]
    finally:
        for k, v in saved.items():
            setattr(env_cfg.env, k, v)
        if "outcome_stats" in vars(env_cfg.env):
            del env_cfg.env.outcome_stats
        for obj, names in ((train_cfg.runner, ("device_rollout", "policy_class_name", "opponent_pool_size", "opponent_pool_recurrent", "opponent_priority",
                                               "num_steps_per_env", "save_interval")), (train_cfg.policy, ("rnn_hidden_size",))):
            for name in names:
                if name in vars(obj):
                    delattr(obj, name)
