"""-m gpu: the recurrent high-level policy of the game tasks on the device path -- ``lg_game_lstm_act`` (include/legged_game_recurrent.h:
the low-level actor and the actor MLP behind the actor memory in one launch, with the command clip) against the separate launches it
replaces and against float64, ``step_policy`` / ``make_graphed_policy_step`` with a ``RecurrentFusedActor`` against their parts on
``high_level_game`` and ``scripted_predator_game``, the runner's device rollout, and ``scripts/play_game.py`` on a recurrent checkpoint.
Nothing here reads outside the tree."""
import copy
import json
import math
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import game_twin as tw
from tests.game_fixtures import game_registered  # noqa: F401
from tests.noise_check import check_noise
from tests.recurrent_ref import actor_forward64, actor_params64
from tests.test_gpu_game import make_game, pack_params, write_ll_checkpoint
from tests.test_gpu_pursuer_game import make_scripted

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EXTRA = 5                    # NaN rows behind row n of h and of every output
HIDDEN = [512, 256, 128]
# last-layer biases and stds in the manner of tests/test_gpu_game_policy.py: every clipped column on both sides of its range (|x| <= 1 for
# columns 0 / 1, <= 2 for 4 / 5), column 2 on both sides of +pi, |z| small enough that the f32 log-prob keeps 2e-5
BIAS = (0.7, -0.7, 2.2, 0.0, 1.5, -1.5)
STD = (0.6, 0.6, 1.0, 1.0, 1.0, 1.0)
# (memory units; hidden widths): fewer tiles than waves / the tasks' default, the 137 KB block / tile counts 3, 5, 7 that 8 waves do not divide
ACTORS = [(32, (32, 32, 32)), (256, (512, 256, 128)), (32, (96, 160, 224))]
ACTOR_IDS = [f"{H}-{'-'.join(map(str, hid))}" for H, hid in ACTORS]


def _policy(H, hidden, nA=6, seed=3, device=DEV):
    """What ``DeviceLstmActor`` reads of an actor-critic: ``.actor`` (Linear / ELU x 3 / Linear, biases uniform in [-1, 1], the last BIAS) and ``.std``."""
    torch.manual_seed(seed)
    dims = (H,) + tuple(hidden) + (nA,)
    mods = []
    for i in range(4):
        lin = nn.Linear(dims[i], dims[i + 1])                 # drawn on the CPU: the same weights with or without a GPU
        with torch.no_grad():
            lin.bias.uniform_(-1.0, 1.0)
            if i == 3:
                lin.bias.copy_(torch.tensor(BIAS[:nA]))
        mods += [lin] + ([nn.ELU()] if i < 3 else [])
    return types.SimpleNamespace(actor=nn.Sequential(*mods).to(device), std=torch.tensor(STD[:nA]).to(device))


_cache = {}


def _hl(H, hidden):
    from legged_games_gym_amd.rl.recurrent_actor import DeviceLstmActor
    if (H, hidden) not in _cache:
        policy = _policy(H, hidden, seed=H + len(hidden))
        _cache[(H, hidden)] = (policy, DeviceLstmActor(policy, DEV, seed=11))
    return _cache[(H, hidden)]


def _ll():
    from legged_games_gym_amd.rl import ActorCritic, FusedActor
    if "ll" not in _cache:
        torch.manual_seed(4)
        ac = ActorCritic(235, 235, 12, actor_hidden_dims=HIDDEN, critic_hidden_dims=HIDDEN).to(DEV)
        _cache["ll"] = (ac, FusedActor(ac, DEV, seed=1))
    return _cache["ll"]


def _guarded(n, width, values=None):
    """[n + EXTRA, width] of NaN (``values`` in the first n rows); returns the full buffer."""
    full = torch.full((n + EXTRA, width) if width else (n + EXTRA,), float("nan"), device=DEV)
    if values is not None:
        full[:n] = values.to(DEV)
    return full


def _inputs(n, H, seed):
    gen = torch.Generator().manual_seed(seed)
    h = _guarded(n, H, torch.rand(n, H, generator=gen) * 2.0 - 1.0)              # a memory's output range
    hl_obs = _guarded(n, 19, torch.randn(n, 19, generator=gen) * 3.0)
    ll_obs = _guarded(n, 235, torch.randn(n, 235, generator=gen) * 1.5)
    return h, hl_obs, ll_obs


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _separate(lib, da, ll, P, h, ll_obs, n, seed, step, ctr, deterministic=False):
    """``lg_lstm_actor_act`` -> ``lg_game_pre`` on a copy, and ``lg_policy_act(ll, deterministic = 1)``."""
    from legged_games_gym_amd import capi
    sample, mean = _guarded(n, 6), _guarded(n, 6)
    assert lib.lg_lstm_actor_act(da.handle, h.data_ptr(), sample.data_ptr(), mean.data_ptr(), n, seed, step, ctr, int(deterministic), _stream()) == 0
    command, llc = sample[:n].clone(), torch.full((n, 4), 7.0, device=DEV)
    capi.game_pre(P, capi.game_buffers({"command": command.data_ptr(), "ll_commands": llc.data_ptr()}), _stream())
    act = _guarded(n, 12)
    assert lib.lg_policy_act(ll.handle, ll_obs.data_ptr(), act.data_ptr(), None, n, seed, step, ctr, 1, _stream()) == 0
    return dict(command=command, ll_commands=llc, mean=mean[:n], sample=sample[:n], ll_actions=act[:n])


def _one_launch(da, ll, P, h, hl_obs, ll_obs, n, seed, step, ctr, deterministic=False, optional=True):
    from legged_games_gym_amd import capi
    out = dict(command=_guarded(n, 6), ll_commands=_guarded(n, 4), ll_actions=_guarded(n, 12), mean=_guarded(n, 6))
    if optional:
        out.update(sample=_guarded(n, 6), sigma=_guarded(n, 6), log_prob=_guarded(n, 0), obs_copy=_guarded(n, 19))
    p = lambda k: out[k].data_ptr() if k in out else None
    B = capi.game_buffers({"command": p("command"), "ll_commands": p("ll_commands")})
    rc = capi.game_lstm_act(da.handle, ll.handle, P, B, h.data_ptr(), hl_obs.data_ptr(), ll_obs.data_ptr(), p("ll_actions"), p("mean"), seed, step, ctr,
                            deterministic, p("sample"), p("sigma"), p("log_prob"), p("obs_copy"), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    for name, t in out.items():
        assert bool(torch.isnan(t[n:]).all()), f"{name}: the guard rows behind row {n} were written"
    return {k: v[:n] for k, v in out.items()}


# ----------------------------------------------------------------------------- 1. bit-identity with the separate launches
@pytest.mark.parametrize("counter_on_device", [False, True], ids=["host_step", "device_counter"])
@pytest.mark.parametrize("heading", [1, 0], ids=["heading", "no_heading"])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 65])
@pytest.mark.parametrize("H,hidden", ACTORS, ids=ACTOR_IDS)
def test_one_launch_is_bit_identical_to_the_separate_launches(H, hidden, n, heading, counter_on_device):
    from legged_games_gym_amd import capi
    lib = capi.load_library()
    assert lib.lg_mlp_wide_set_precision(-1) == 1                                  # the default; an invalid mode only reads it
    (policy, da), (_, ll) = _hl(H, hidden), _ll()
    h, hl_obs, ll_obs = _inputs(n, H, seed=100 + n)
    P = pack_params(tw.params(num_envs=n, heading_command=heading))
    step_value = 77 + n
    counter = torch.tensor([step_value - 1], dtype=torch.int64, device=DEV)        # the kernels read counter + 1
    step, ctr = (-1, counter.data_ptr()) if counter_on_device else (step_value, None)
    seed = 4242
    want = _separate(lib, da, ll, P, h, ll_obs, n, seed, step, ctr)
    got = _one_launch(da, ll, P, h, hl_obs, ll_obs, n, seed, step, ctr)
    for name in ("command", "ll_commands", "mean", "sample", "ll_actions"):
        assert torch.equal(got[name], want[name]), (name, float((got[name] - want[name]).abs().max()))
    assert torch.equal(got["obs_copy"], hl_obs[:n]) and torch.equal(got["ll_commands"], got["command"][:, :4])
    assert int(counter[0]) == step_value - 1
    assert torch.equal(got["sigma"], policy.std.expand(n, 6))
    assert torch.equal(got["command"][:, 3], got["sample"][:, 3]) and float((got["sample"] - got["mean"]).abs().max()) > 0.0
    if not heading:
        assert torch.equal(got["command"][:, 2], got["sample"][:, 2])

    # the optional outputs are optional; deterministic: the command is the clipped mean
    bare = _one_launch(da, ll, P, h, hl_obs, ll_obs, n, seed, step, ctr, optional=False)
    for name in ("command", "ll_commands", "mean", "ll_actions"):
        assert torch.equal(bare[name], got[name]), name
    det = _one_launch(da, ll, P, h, hl_obs, ll_obs, n, seed, step, ctr, deterministic=True)
    det_w = _separate(lib, da, ll, P, h, ll_obs, n, seed, step, ctr, deterministic=True)
    clipped_mean, llc = got["mean"].clone(), torch.empty(n, 4, device=DEV)
    capi.game_pre(P, capi.game_buffers({"command": clipped_mean.data_ptr(), "ll_commands": llc.data_ptr()}), _stream())
    torch.cuda.synchronize()
    assert torch.equal(det["command"], clipped_mean) and torch.equal(det["mean"], got["mean"]) and torch.equal(det["sample"], got["mean"])
    assert torch.equal(det["command"], det_w["command"]) and torch.equal(det["ll_actions"], got["ll_actions"])


# ----------------------------------------------------------------------------- 2. clip and wrap really exercised
@pytest.mark.parametrize("heading", [1, 0], ids=["heading", "no_heading"])
def test_clip_and_wrap_are_exercised_on_both_sides(heading):
    """n = 65 with BIAS / STD: every clipped column has samples outside and inside its range, column 2 samples beyond +-pi and inside --
    asserted before what happened to them is."""
    H, hidden = ACTORS[1]
    n = 65
    (policy, da), (_, ll) = _hl(H, hidden), _ll()
    h, hl_obs, ll_obs = _inputs(n, H, seed=100 + n)
    P = pack_params(tw.params(num_envs=n, heading_command=heading))
    got = _one_launch(da, ll, P, h, hl_obs, ll_obs, n, 4242, 142, None)
    sample, command = got["sample"], got["command"]
    for col, hi in ((0, 1.0), (1, 1.0), (4, 2.0), (5, 2.0)):
        out = sample[:, col].abs() > hi
        assert bool(out.any()) and bool((~out).any()), col
        assert bool((command[out][:, col].abs() == hi).all()) and torch.equal(command[~out][:, col], sample[~out][:, col]), col
        assert torch.equal(torch.sign(command[out][:, col]), torch.sign(sample[out][:, col])), col
    beyond = sample[:, 2].abs() > math.pi
    assert bool(beyond.any()) and bool((~beyond).any())
    if heading:
        assert bool((command[beyond][:, 2].abs() <= math.pi).all()) and not torch.equal(command[:, 2], sample[:, 2])
        turn = (sample[beyond][:, 2].double() - command[beyond][:, 2].double()) / (2.0 * math.pi)
        assert float((turn - turn.round()).abs().max()) < 1e-6                      # the same angle, a whole number of turns away
    else:
        assert torch.equal(command[:, 2], sample[:, 2])
    want, want_ll = tw.pre(tw.params(num_envs=n, heading_command=heading), sample.cpu().numpy())      # the NumPy twin of lg_game_pre
    assert np.array_equal(command.cpu().numpy(), want) and np.array_equal(got["ll_commands"].cpu().numpy(), want_ll)


# ----------------------------------------------------------------------------- 3. against float64 outside any kernel
def test_one_launch_matches_float64_forwards_and_log_prob():
    """n = 33 (a second workgroup per role) at the tasks' default actor: the high-level means within 2e-5 of the output scale of
    ``actor_forward64`` (the bar of tests/test_gpu_recurrent_actor.py for this arithmetic), the low-level actions within 1e-4 (the
    split-bf16 bar of test_shared_actor_launch_matches_float64_forwards), ``log_prob`` within 2e-5 of a float64 Normal log-prob of
    (``sample``, ``mean``, std)."""
    H, hidden = ACTORS[1]
    n = 33
    (policy, da), (ll_ac, ll) = _hl(H, hidden), _ll()
    h, hl_obs, ll_obs = _inputs(n, H, seed=133)
    got = _one_launch(da, ll, pack_params(tw.params(num_envs=n)), h, hl_obs, ll_obs, n, 4242, 110, None)
    for name, key, layers, x, tol in (("high-level mean", "mean", policy.actor, h[:n], 2e-5), ("low-level actions", "ll_actions", ll_ac.actor, ll_obs[:n], 1e-4)):
        want = actor_forward64(*actor_params64(layers), x.cpu().double().numpy())
        err, scale = float(np.abs(got[key].cpu().double().numpy() - want).max()), max(1.0, float(np.abs(want).max()))
        print(f"[observed] k_game_lstm_act n {n} {name}: err {err:.3e}, scale {scale:.3f}, err / scale {err / scale:.3e} (bar {tol:g})")
        assert err < tol * scale, (name, err, scale)
    sample, mean, std = got["sample"].cpu().double(), got["mean"].cpu().double(), policy.std.cpu().double()
    z = (sample - mean) / std
    want_lp = (-0.5 * z * z - std.log() - 0.5 * math.log(2.0 * math.pi)).sum(-1)
    err = float((got["log_prob"].cpu().double() - want_lp).abs().max())
    print(f"[observed] k_game_lstm_act n {n} log_prob: err {err:.3e}, max |z| {float(z.abs().max()):.2f} (bar 2e-5)")
    assert err < 2e-5, err


# ----------------------------------------------------------------------------- 4. noise
def test_noise_is_the_reference_philox_stream():
    """``sample - mean`` of the six actions is ``std * eps`` of the NumPy Philox reference for (seed; env, step), with the step from the
    host and from a device counter holding step - 1."""
    H, hidden = ACTORS[0]
    n, seed = 37, 9
    (policy, da), (_, ll) = _hl(H, hidden), _ll()
    h, hl_obs, ll_obs = _inputs(n, H, seed=6)
    P = pack_params(tw.params(num_envs=n))
    std = policy.std.cpu().double().numpy()
    report = {}
    for step in (41, 2 ** 32 + 4242):
        got = _one_launch(da, ll, P, h, hl_obs, ll_obs, n, seed, step, None)
        check_noise(got["sample"].cpu().numpy(), got["mean"].cpu().numpy(), std, seed, step, report)
    c = 776
    counter = torch.tensor([c], dtype=torch.int64, device=DEV)
    got = _one_launch(da, ll, P, h, hl_obs, ll_obs, n, seed, -1, counter.data_ptr())
    check_noise(got["sample"].cpu().numpy(), got["mean"].cpu().numpy(), std, seed, c + 1, report)
    assert int(counter[0]) == c
    by_host = _one_launch(da, ll, P, h, hl_obs, ll_obs, n, seed, c + 1, None)
    assert torch.equal(by_host["sample"], got["sample"])
    print("[observed] k_game_lstm_act noise: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(report.items())))


# ----------------------------------------------------------------------------- env fixtures
def _recurrent_policy(units=64, hidden=(64, 64, 32), seed=6):
    from legged_games_gym_amd.rl import ActorCriticRecurrent
    torch.manual_seed(seed)
    ac = ActorCriticRecurrent(19, 19, 6, actor_hidden_dims=list(hidden), critic_hidden_dims=list(hidden), rnn_hidden_size=units).to(DEV)
    with torch.no_grad():
        ac.std.copy_(torch.tensor(STD))
        ac.actor[-1].bias.copy_(torch.tensor(BIAS))
    return ac


def _two_envs(tmp_path, make, seed=9, reset_seed=90, n=64):
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)         # a random low-level policy
    A, B = make(ckpt, n, seed=seed), make(ckpt, n, seed=seed)
    for env in (A, B):
        torch.manual_seed(reset_seed)                                              # reset_idx from the host draws from torch's generator
        env.reset()
    assert torch.equal(A.obs_buf, B.obs_buf) and torch.equal(A.ll_env.root_states, B.ll_env.root_states) and torch.equal(A.predator_pos, B.predator_pos)
    return A, B


def _assert_same_state(A, B, k):
    for name in ("obs_buf", "rew_buf", "reset_buf", "predator_pos", "curr_episode_step"):
        assert torch.equal(getattr(A, name), getattr(B, name)), (k, name)
    assert torch.equal(A.ll_env.root_states, B.ll_env.root_states) and torch.equal(A.ll_env.obs_buf, B.ll_env.obs_buf), k
    assert torch.equal(A.ll_env.commands, B.ll_env.commands), k


def _same_memories(fa, fb):
    return all(torch.equal(x, y) for pa, pb in zip(fa.hidden_states(), fb.hidden_states()) for x, y in zip(pa, pb))


# ----------------------------------------------------------------------------- 5. fallback
def test_env_takes_the_separate_launches_at_precision_0_on_rc_minus_4_and_without_the_library(tmp_path, monkeypatch, capsys):
    from legged_games_gym_amd import capi
    from legged_games_gym_amd.rl.recurrent_actor import DeviceLstmActor, RecurrentFusedActor
    lib = capi.load_library()
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    env = make_game(ckpt, 64, seed=9)
    env.reset()
    rfa = RecurrentFusedActor(_recurrent_policy(), DEV, seed=21, num_envs=64)
    obs_in, obs_out = env.obs_buf, env._obs_pair[env._obs_flip ^ 1]
    launches = []
    real = capi.game_lstm_act
    monkeypatch.setattr(capi, "game_lstm_act", lambda *a, **k: launches.append(real(*a, **k)) or launches[-1])

    def act():
        rfa.reset_states()
        rfa._flip, rfa.fused._host_step = 0, 0
        obs_out.fill_(float("nan"))
        sample, sigma, logp = torch.empty(64, 6, device=DEV), torch.empty(64, 6, device=DEV), torch.empty(64, device=DEV)
        command, mean, ll_actions, _ = env._act(rfa, obs_in, obs_out, False, sample, sigma, logp)
        torch.cuda.synchronize()
        assert rfa.fused._host_step == 1 and torch.equal(obs_out, obs_in)
        return [t.clone() for t in (command, mean, sample, sigma, logp, ll_actions, env.ll_env.commands)]

    capsys.readouterr()
    want = act()
    assert launches == [0] and capsys.readouterr().out == ""                        # the one launch, not a word
    assert env.shared_actor_launch(rfa) is True and rfa.fused._host_step == 1      # (answers for the recurrent actor; does not count a step)
    del launches[:]

    def check(got, tag, same_ll):
        for i, name in enumerate(("command", "mean", "sample", "sigma")):
            assert torch.equal(got[i], want[i]), (tag, name)
        assert float((got[4] - want[4]).abs().max()) < 2e-5, tag                    # (the log-prob of the separate launches is torch's)
        assert torch.equal(got[6], want[6]), tag
        assert torch.equal(got[5], want[5]) == same_ll, tag

    old = lib.lg_mlp_wide_set_precision(0)
    try:
        got = act()
        out = capsys.readouterr().out
        assert launches == [] and out.count("\n") == 1 and "wide precision 0" in out and "lg_lstm_actor_act" in out, out
        check(got, "precision 0", same_ll=False)                                   # (the low-level actor is then the exact-f32 kernel)
        assert env.shared_actor_launch(rfa) is False
        act()
        assert capsys.readouterr().out == ""                                       # said once
    finally:
        lib.lg_mlp_wide_set_precision(old)
    assert lib.lg_mlp_wide_set_precision(-1) == 1

    # rc -4: the library is handed the handle of a 2-action actor where the env's call names its own
    two = DeviceLstmActor(_policy(64, (64, 64, 32), nA=2), DEV, seed=21)
    monkeypatch.setattr(capi, "game_lstm_act", lambda hl, *a, **k: launches.append(real(two.handle, *a, **k)) or launches[-1])
    got = act()
    out = capsys.readouterr().out
    assert launches == [-4] and out.count("\n") == 1 and "no kernel for this actor pair" in out, out
    check(got, "rc -4", same_ll=True)
    monkeypatch.setattr(capi, "game_lstm_act", real)

    # without the library
    monkeypatch.setattr(capi.LIBRARIES["game_recurrent"], "handle", None)
    monkeypatch.setenv("LG_GAME_RECURRENT_LIB", str(tmp_path / "absent.so"))
    got = act()
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "absent.so" in out and "lg_lstm_actor_act" in out, out
    check(got, "no library", same_ll=True)


# ----------------------------------------------------------------------------- 6. step_policy against the pieces
@pytest.mark.parametrize("task", ["high_level_game", "scripted_predator_game"])
def test_step_policy_equals_its_pieces_and_the_graphed_step_the_eager_one(tmp_path, task):
    """A: ``step_policy(RecurrentFusedActor)``.  B, identically seeded: ``step_memories`` -> ``lg_lstm_actor_act`` -> ``env.step(command)``.
    Two steps with a reset forced in between; then four replays of the graphed policy step on A against four eager ``step_policy`` on B."""
    from legged_games_gym_amd.rl.recurrent_actor import RecurrentFusedActor
    make = make_game if task == "high_level_game" else make_scripted
    A, B = _two_envs(tmp_path, make)
    assert type(A).__name__ == {"high_level_game": "HighLevelGame", "scripted_predator_game": "ScriptedPredatorGame"}[task]
    ac = _recurrent_policy()
    fa, fb = RecurrentFusedActor(ac, DEV, seed=21, num_envs=64), RecurrentFusedActor(ac, DEV, seed=21, num_envs=64)
    forced = torch.arange(3, 64, 5, device=DEV)
    sample = torch.empty(64, 6, device=DEV)
    for k in range(2):
        prev_a, obs_b, flags = A.obs_buf, B.obs_buf, B.reset_buf.clone()
        (ca, ma, hca), (oa, _, ra, da, _) = A.step_policy(fa, sample=sample, with_critic_memory=True)
        h_a, h_c = fb.step_memories(obs_b, obs_b, reset=B.reset_buf)
        actions, mb = fb.fused.act_with_mean(h_a)
        raw = actions.clone()
        ob, _, rb, db, _ = B.step(actions)                                         # clips `actions` where it is
        torch.cuda.synchronize()
        assert torch.equal(ca, actions) and torch.equal(ma, mb) and torch.equal(sample, raw) and torch.equal(hca, h_c), k
        assert oa is A.obs_buf and oa is not prev_a and torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db), k
        _assert_same_state(A, B, k)
        assert _same_memories(fa, fb) and fa.fused._host_step == fb.fused._host_step == k + 1
        assert A.ll_env.common_step_counter == B.ll_env.common_step_counter and A._obs_flip == B._obs_flip
        if k == 1:                                                                 # a reset row's memory started from zero
            fresh = RecurrentFusedActor(ac, DEV, seed=21, num_envs=64)
            fresh.step_memories(obs_b, obs_b)
            rows = flags.nonzero().flatten()
            assert set(forced.tolist()) <= set(rows.tolist()) and len(rows) < 64
            for mine, zero in zip(fa.hidden_states(), fresh.hidden_states()):
                for x, y in zip(mine, zero):
                    assert torch.equal(x[0, rows], y[0, rows])
            live = (~flags).nonzero().flatten()
            assert not torch.equal(fa.hidden_states()[0][0][0, live], fresh.hidden_states()[0][0][0, live])
        for env in (A, B):                                                         # the reset forced in between
            env.reset_buf[forced] = True

    # the graphed policy step: memories from zero on the sims' device step counters
    ga = RecurrentFusedActor(ac, DEV, seed=21, step_counter=A.ll_env._sim.buf["step_counter"], num_envs=64)
    gb = RecurrentFusedActor(ac, DEV, seed=21, step_counter=B.ll_env._sim.buf["step_counter"], num_envs=64)
    with pytest.raises(ValueError):
        A.make_graphed_policy_step(fa)                                             # a host-counted noise stream cannot be replayed
    replay = A.make_graphed_policy_step(ga, warmup=3)
    for _ in range(3):
        B.step_policy(gb)
    for k in range(4):
        oa, _, ra, da, _ = replay()
        (cb, mb), (ob, _, rb, db, _) = B.step_policy(gb)
        torch.cuda.synchronize()
        ca, ma = ga.output_buffers(64)
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db) and torch.equal(ca, cb) and torch.equal(ma, mb), k
        _assert_same_state(A, B, k)
        assert _same_memories(ga, gb), k
        for env in (A, B):
            assert int(env.ll_env._sim.buf["step_counter"][0]) == env.ll_env.common_step_counter
    assert float(ga.hidden_states()[0][0].abs().max()) > 0.0 and float(ga.hidden_states()[1][0].abs().max()) > 0.0


# ----------------------------------------------------------------------------- 7. / 8. the runner and play_game
def _game_runner(reg, tmp_path, monkeypatch, ckpt, n=64, units=64, **runner_keys):
    import legged_games_gym_amd.utils.task_registry as tr_mod
    from legged_games_gym_amd.utils import get_args
    from legged_games_gym_amd.utils.helpers import apply_policy_args
    monkeypatch.setattr(tr_mod, "LEGGED_GYM_ROOT_DIR", str(tmp_path))
    env_cfg, train_cfg = reg.get_cfgs("high_level_game")
    env_cfg.terrain.mesh_type, env_cfg.env.ll_policy_path = "plane", ckpt
    for key in ("graphed_rollout",):
        if hasattr(train_cfg.runner, key):
            delattr(train_cfg.runner, key)
    train_cfg.runner.device_rollout = True                                  # a runner key, not a config field: set on this registration only
    for key, value in runner_keys.items():
        setattr(train_cfg.runner, key, value)
    args = get_args(["--task", "high_level_game", "--num_envs", str(n), "--headless", "--sim_device", DEV, "--rl_device", DEV,
                     "--policy_class_name", "ActorCriticRecurrent", "--rnn_hidden_size", str(units)])
    apply_policy_args(train_cfg, args)
    assert train_cfg.runner.num_steps_per_env == 24
    env, _ = reg.make_env("high_level_game", args)
    torch.manual_seed(1234)                                                  # the same initial policy on every runner
    runner, _ = reg.make_alg_runner(env, "high_level_game", args)
    # episodes that end inside each of the first two rollouts: low-level time-outs 3 .. 43 steps ahead on every other env
    env.ll_env.episode_length_buf[::2] = int(env.ll_env.max_episode_length) - 3 - (torch.arange(0, n, 2, device=DEV) % 41)
    return env, runner


def _stats(runner):
    N, dev = runner.env.num_envs, runner.device
    sums = torch.zeros(3, device=dev)
    return {"cur_rew": torch.zeros(N, device=dev), "cur_len": torch.zeros(N, device=dev), "sum_rew": sums[0], "sum_len": sums[1], "count": sums[2], "_sums": sums}


def _snapshot(st):
    keep = [st.observations, st.actions, st.mu, st.sigma, st.actions_log_prob, st.values, st.rewards, st.dones] + list(st.initial_hidden_a) + list(st.initial_hidden_c)
    return [t.clone() for t in keep]


def _check_storage_against_batch_mode(runner, tag):
    """``_check_storage_against_batch_mode`` of tests/test_gpu_recurrent.py at its bars (2e-5 of the output scale) for the means and the
    values; the log-prob belongs to the unclipped sample here and is checked where the samples are drawn again."""
    st, ac = runner.alg.storage, runner.alg.actor_critic
    assert int(st.dones.sum()) > 0, "no episode ended in the rollout: the reset path went untested"
    with torch.no_grad():
        (obs, cobs, act, val, adv, ret, lp, mu, sig, (hid_a, hid_c), masks), = list(st.recurrent_mini_batch_generator(1, 1))
        ac64 = copy.deepcopy(ac).double()
        d = lambda hid: tuple(x.double() for x in hid)
        ac64.act(obs.double(), masks=masks, hidden_states=d(hid_a))
        new_mu = ac64.action_mean
        new_val = ac64.evaluate(cobs.double(), masks=masks, hidden_states=d(hid_c))
    e_mu, e_val = float((new_mu - mu).abs().max()), float((new_val - val).abs().max())
    s_mu, s_val = max(1.0, float(new_mu.abs().max())), max(1.0, float(new_val.abs().max()))
    print(f"[observed] {tag}: mu err {e_mu:.3e} (scale {s_mu:.2f})  value err {e_val:.3e} (scale {s_val:.2f})  dones {int(st.dones.sum())}")
    assert e_mu < 2e-5 * s_mu and e_val < 2e-5 * s_val, (tag, e_mu, e_val)


def test_runner_device_rollout_with_a_recurrent_policy(tmp_path, monkeypatch, game_registered, capsys):
    from legged_games_gym_amd.rl.recurrent_actor import DeviceLstmActor, RecurrentFusedActor
    from legged_games_gym_amd.scripts import play_game as pg
    reg = game_registered
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    env_g, run_g = _game_runner(reg, tmp_path, monkeypatch, ckpt)
    env_e, run_e = _game_runner(reg, tmp_path, monkeypatch, ckpt, graphed_rollout=False)
    for runner in (run_g, run_e):
        assert isinstance(runner._fused, RecurrentFusedActor) and runner._game_rollout and runner._recurrent_rollout
    assert torch.equal(env_g.obs_buf, env_e.obs_buf) and env_g.common_step_counter == env_e.common_step_counter
    T, N = run_g.num_steps_per_env, env_g.num_envs
    assert T == 24 and N == 64 and run_g.alg.actor_critic.memory_a.rnn.hidden_size == 64

    # captured: one eager warm-up rollout (discarded), then the capture, then one replay; eager: the same two rollouts as plain launches
    graphed = run_g._try_build_graphed_rollout()
    assert graphed is not None and run_e._try_build_graphed_rollout() is None, capsys.readouterr().out
    with torch.inference_mode():
        graphed[0].replay()
    env_g.common_step_counter += T
    run_g.alg.storage.step = T
    stats = _stats(run_e)
    with torch.inference_mode():
        run_e._rollout_steps(stats)
        _check_storage_against_batch_mode(run_e, "eager, first rollout")
        run_e.alg.storage.clear()
        obs_e, _ = run_e._rollout_steps(stats)
    torch.cuda.synchronize()
    sg, se = run_g.alg.storage, run_e.alg.storage
    assert float(sg.initial_hidden_a[0].abs().max()) > 0.0                        # the second rollout: a carried-in state
    for i, (a, b) in enumerate(zip(_snapshot(sg), _snapshot(se))):
        assert torch.equal(a, b), f"storage tensor {i} differs between the graph replay and the eager rollouts"
    assert torch.equal(graphed[2], obs_e) and env_g.common_step_counter == env_e.common_step_counter
    for a, b in zip([t for pair in run_g.alg.actor_critic.get_hidden_states() for t in pair], [t for pair in run_e.alg.actor_critic.get_hidden_states() for t in pair]):
        assert torch.equal(a, b)                                                   # the torch memories were refreshed from the same device state
    _check_storage_against_batch_mode(run_g, "graphed, second rollout")

    # storage semantics of the generic path: actions[t] is the clipped command, actions_log_prob[t] the unclipped sample's.  The samples
    # are not stored: a copy of the actor with a zero output layer has mean 0, so its actions are std * eps of the same stream
    ac0 = copy.deepcopy(run_g.alg.actor_critic)
    with torch.no_grad():
        ac0.actor[-1].weight.zero_(); ac0.actor[-1].bias.zero_()
    noise_actor, fused = DeviceLstmActor(ac0, DEV, seed=1), run_g._fused
    h0 = torch.zeros(N, 64, device=DEV)
    noise = torch.empty(T, N, 6, device=DEV)
    for t in range(T):
        step = env_g.common_step_counter - T + t + 1
        assert noise_actor.lib.lg_lstm_actor_act(noise_actor.handle, h0.data_ptr(), noise[t].data_ptr(), None, N, fused.seed, step, None, 0, _stream()) == 0
    torch.cuda.synchronize()
    act, mu, sigma, lp = sg.actions, sg.mu, sg.sigma, sg.actions_log_prob[..., 0]
    sample = mu + noise
    assert torch.equal(sigma, run_g.alg.actor_critic.std.detach().expand_as(sigma))
    want = torch.from_numpy(np.stack([tw.pre(tw.params(num_envs=N, heading_command=1), sample[t].cpu().numpy())[0] for t in range(T)])).to(DEV)
    assert env_g._P.heading_command == 1 and torch.equal(act, want)                # the stored action is the clipped / wrapped sample
    z = (sample.double() - mu.double()) / sigma.double()
    lp_of_sample = (-0.5 * z * z - sigma.double().log() - 0.5 * math.log(2.0 * math.pi)).sum(-1)
    e_lp = float((lp.double() - lp_of_sample).abs().max())
    moved = (sample != act).any(-1)
    print(f"[observed] runner storage: log-prob err {e_lp:.3e} against the unclipped sample; rows with a clip or wrap {int(moved.sum())} of {moved.numel()}")
    assert e_lp < 2e-5 and bool(moved.any()) and bool((~moved).any())
    za = (act.double() - mu.double()) / sigma.double()
    lp_of_stored = (-0.5 * za * za - sigma.double().log() - 0.5 * math.log(2.0 * math.pi)).sum(-1)
    assert float((lp.double() - lp_of_stored)[moved].abs().max()) > 1e-3             # ... not the stored action's

    # two iterations of learn: finite losses, moved LSTM weights; not a word about anything unavailable
    run_g.alg.storage.clear()
    ac = run_g.alg.actor_critic
    before = ac.memory_a.rnn.weight_hh_l0.clone(), ac.memory_c.rnn.weight_ih_l0.clone()
    losses, update = [], run_g.alg.update
    monkeypatch.setattr(run_g.alg, "update", lambda: losses.append(update()) or losses[-1])
    run_g.learn(2)
    torch.cuda.synchronize()
    assert len(losses) == 2 and all(math.isfinite(float(v)) for pair in losses for v in pair), losses
    assert all(bool(torch.isfinite(p).all()) for p in ac.parameters())
    assert not torch.equal(before[0], ac.memory_a.rnn.weight_hh_l0) and not torch.equal(before[1], ac.memory_c.rnn.weight_ih_l0)
    assert "unavailable" not in capsys.readouterr().out

    # play_game on the checkpoint: the graphed policy step on the recurrent policy
    run_dir = run_g.log_dir
    assert os.path.isfile(os.path.join(run_dir, "model_2.pt"))
    args = pg._args(["--task", "high_level_game", "--num_envs", "16", "--steps", "12", "--headless", "--sim_device", DEV, "--rl_device", DEV,
                     "--policy_class_name", "ActorCriticRecurrent", "--rnn_hidden_size", "64", "--load_run", os.path.basename(run_dir)])
    env_p, result, path = pg.play_game(args, steps=args.steps)
    assert path == os.path.join(run_dir, "outcomes_2.json") and json.load(open(path)) == json.loads(json.dumps(result))
    assert result["path"] == "graphed policy step" and result["iteration"] == 2 and result["steps"] == 12 and result["num_envs"] == 16
    assert torch.isfinite(env_p.obs_buf).all()


def test_runner_falls_back_for_a_memory_the_cell_does_not_cover_and_still_learns(tmp_path, monkeypatch, game_registered, capsys):
    reg = game_registered
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    capsys.readouterr()
    env, runner = _game_runner(reg, tmp_path, monkeypatch, ckpt, units=512)
    out = capsys.readouterr().out
    assert runner._fused is None and not runner._game_rollout and not runner._recurrent_rollout
    assert "device rollout unavailable" in out and "512" in out and "generic VecEnv loop" in out, out
    before = runner.alg.actor_critic.memory_a.rnn.weight_hh_l0.clone()
    runner.learn(1)
    assert not torch.equal(before, runner.alg.actor_critic.memory_a.rnn.weight_hh_l0)
