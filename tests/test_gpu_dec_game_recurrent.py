"""-m gpu: recurrent policies on the device path of ``dec_high_level_game`` -- ``lg_dec_lstm_step`` (include/legged_dec_game_recurrent.h: up
to four memories in one launch) against ``lg_lstm_step`` with each role alone and against float64, ``lg_dec_game_lstm_act`` (the three
actors of a step and the command clips in one launch) against the separate launches it replaces, the NumPy twin of the clips, float64 and
the Philox reference.  Nothing here reads outside the tree."""
import math
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import dec_game_twin as dt
from tests.noise_check import check_noise
from tests.recurrent_ref import actor_forward64, actor_params64, lstm_params64, lstm_step64
from tests.test_gpu_dec_game import pack_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-5                   # the cell's bar of tests/test_gpu_recurrent.py
EXTRA = 5                    # NaN rows behind row n of every input and output
HIDDEN = [512, 256, 128]
SIZES = [1, 31, 32, 33, 65]  # one row; one short of, exactly and one past a workgroup's 32 rows; a third workgroup
# last-layer biases and stds: every clipped column on both sides of its range (|x| <= 1 for the prey's columns 0 / 1, <= 2 for the
# predator's), the prey's column 2 on both sides of +pi, |z| small enough that the f32 log-prob keeps 2e-5
BIAS_PREY, STD_PREY = (0.7, -0.7, 2.2, 0.0), (0.6, 0.6, 1.0, 1.0)
BIAS_PRED, STD_PRED = (1.5, -1.5), (1.0, 1.0)
# (memory units; hidden widths): fewer tiles than waves / the task's default, the 137 KB block / tile counts 3, 5, 7 that 8 waves do not divide
ACTORS = [(32, (32, 32, 32)), (256, (512, 256, 128)), (32, (96, 160, 224))]
ACTOR_IDS = [f"{H}-{'-'.join(map(str, hid))}" for H, hid in ACTORS]
SEED_PRED, SEED_PREY = 4242 + 104729, 4242

_cache = {}


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _guarded(n, width, values=None):
    """[n + EXTRA, width] of NaN (``values`` in the first n rows)."""
    full = torch.full((n + EXTRA, width) if width else (n + EXTRA,), float("nan"), device=DEV)
    if values is not None:
        full[:n] = values.to(DEV)
    return full


# ----------------------------------------------------------------------------- 1. the cell launch
ROLE_IN = (3, 3, 16, 16)     # predator actor / critic memory read the predator's 3 observations, the prey's two its 16
ROLE_SETS = [(0,), (1,), (0, 1, 2), (0, 2), (0, 1, 2, 3)]
UNITS = {"32": (32, 32, 32, 32), "256": (256, 256, 256, 256), "mixed": (32, 32, 256, 256)}


def _memories(units):
    """Four ``DeviceLstm`` (and their modules) of ``units[r]`` units on ``ROLE_IN[r]`` inputs, drawn on the CPU."""
    from legged_games_gym_amd.rl.recurrent_actor import DeviceLstm
    if ("mem", units) not in _cache:
        rnns = []
        for r in range(4):
            torch.manual_seed(10 + r)
            rnns.append(nn.LSTM(ROLE_IN[r], units[r]).to(DEV))
        _cache[("mem", units)] = (rnns, [DeviceLstm(rnn, DEV) for rnn in rnns])
    return _cache[("mem", units)]


def _cell_case(units, n):
    """Inputs of the four roles at ``n`` rows (NaN in the stale state of reset rows and in the guard rows) and, computed once and left
    unchanged, what ``lg_lstm_step`` gives for each role alone."""
    from legged_games_gym_amd import capi
    from legged_games_gym_amd.rl.recurrent_actor import lstm_step
    key = ("cell", units, n)
    if key not in _cache:
        _, cells = _memories(units)
        gen = torch.Generator().manual_seed(1000 * n + sum(units))
        reset = torch.zeros(n + EXTRA, dtype=torch.uint8)
        reset[:n] = (torch.arange(n) % 3 == 1).to(torch.uint8)
        reset[n:] = 1
        reset = reset.to(DEV)
        x, h, c, want = [], [], [], []
        for r in range(4):
            x.append(_guarded(n, ROLE_IN[r], torch.rand(n, ROLE_IN[r], generator=gen) * 6.0 - 3.0))
            for dst in (h, c):
                t = _guarded(n, units[r], torch.rand(n, units[r], generator=gen) * 2.0 - 1.0)
                t[:n][reset[:n] != 0] = float("nan")
                dst.append(t)
            ho, co = _guarded(n, units[r]), _guarded(n, units[r])
            lstm_step(capi.load_library(), cells[r], None, x[r], None, reset, (h[r], c[r]), (ho, co), None, None, n, _stream())
            torch.cuda.synchronize()
            assert bool(torch.isfinite(ho[:n]).all()) and bool(torch.isnan(ho[n:]).all())
            want.append((ho, co))
        _cache[key] = (x, h, c, reset, want)
    return _cache[key]


def _dec_step(units, n, roles):
    from legged_games_gym_amd import capi
    _, cells = _memories(units)
    x, h, c, reset, _ = _cell_case(units, n)
    outs = [(_guarded(n, units[r]), _guarded(n, units[r])) for r in range(4)]
    capi.dec_lstm_step([(cells[r].handle, x[r].data_ptr(), h[r].data_ptr(), c[r].data_ptr(), outs[r][0].data_ptr(), outs[r][1].data_ptr())
                        if r in roles else None for r in range(4)], reset.data_ptr(), n, _stream())
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("roles", ROLE_SETS, ids=lambda r: "roles" + "".join(map(str, r)))
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("units", list(UNITS), ids=lambda u: "units" + u)
def test_cell_launch_is_bit_identical_to_each_role_alone(units, n, roles):
    units = UNITS[units]
    *_, want = _cell_case(units, n)
    outs = _dec_step(units, n, roles)
    for r in range(4):
        for got, ref, name in zip(outs[r], want[r], ("h", "c")):
            if r in roles:
                assert torch.equal(got[:n], ref[:n]), (r, name, float((got[:n] - ref[:n]).abs().max()))
                assert bool(torch.isnan(got[n:]).all()), (r, name, "guard rows written")
            else:
                assert bool(torch.isnan(got).all()), (r, name, "an absent role's buffer was written")


def test_cell_launch_matches_float64():
    """n = 33 (a second workgroup per role), all four roles, 32 and 256 units in one launch, against ``lstm_step64``."""
    units, n = UNITS["mixed"], 33
    rnns, _ = _memories(units)
    x, h, c, reset, _ = _cell_case(units, n)
    outs = _dec_step(units, n, (0, 1, 2, 3))
    flags = reset[:n].cpu().numpy()
    for r in range(4):
        clean = lambda t: torch.nan_to_num(t[:n], nan=0.0).cpu().numpy()             # (a reset row's stale state is not read)
        want = lstm_step64(lstm_params64(rnns[r]), x[r][:n].cpu().numpy(), clean(h[r]), clean(c[r]), flags)
        for got, ref, name in zip(outs[r], want, ("h", "c")):
            err, scale = float(np.abs(got[:n].cpu().double().numpy() - ref).max()), max(1.0, float(np.abs(ref).max()))
            print(f"[observed] k_dec_lstm_cell n {n} role {r} ({ROLE_IN[r]} -> {units[r]}) {name}: err {err:.3e}, scale {scale:.3f} (bar {TOL:g})")
            assert err < TOL * scale, (r, name, err)


# ----------------------------------------------------------------------------- 2. the actor launch
def _policy(H, hidden, bias, std, seed):
    """What ``DeviceLstmActor`` reads of an actor-critic: ``.actor`` (Linear / ELU x 3 / Linear, biases uniform in [-1, 1], the last ``bias``) and ``.std``."""
    torch.manual_seed(seed)
    dims = (H,) + tuple(hidden) + (len(bias),)
    mods = []
    for i in range(4):
        lin = nn.Linear(dims[i], dims[i + 1])                 # drawn on the CPU: the same weights with or without a GPU
        with torch.no_grad():
            lin.bias.uniform_(-1.0, 1.0)
            if i == 3:
                lin.bias.copy_(torch.tensor(bias))
        mods += [lin] + ([nn.ELU()] if i < 3 else [])
    return types.SimpleNamespace(actor=nn.Sequential(*mods).to(DEV), std=torch.tensor(std).to(DEV))


def _agents(H, hidden):
    """((predator policy, its DeviceLstmActor), (prey policy, its DeviceLstmActor))."""
    from legged_games_gym_amd.rl.recurrent_actor import DeviceLstmActor
    if ("agents", H, hidden) not in _cache:
        pred, prey = _policy(H, hidden, BIAS_PRED, STD_PRED, seed=H + 5), _policy(H, hidden, BIAS_PREY, STD_PREY, seed=H + 3)
        _cache[("agents", H, hidden)] = ((pred, DeviceLstmActor(pred, DEV, seed=12)), (prey, DeviceLstmActor(prey, DEV, seed=11)))
    return _cache[("agents", H, hidden)]


def _ll():
    from legged_games_gym_amd.rl import ActorCritic, FusedActor
    if "ll" not in _cache:
        torch.manual_seed(4)
        ac = ActorCritic(235, 235, 12, actor_hidden_dims=HIDDEN, critic_hidden_dims=HIDDEN).to(DEV)
        _cache["ll"] = (ac, FusedActor(ac, DEV, seed=1))
    return _cache["ll"]


def _inputs(n, H, seed):
    gen = torch.Generator().manual_seed(seed)
    t = dict(h_pred=_guarded(n, H, torch.rand(n, H, generator=gen) * 2.0 - 1.0), h_prey=_guarded(n, H, torch.rand(n, H, generator=gen) * 2.0 - 1.0),
             pred_obs=_guarded(n, 3, torch.randn(n, 3, generator=gen) * 3.0), prey_obs=_guarded(n, 16, torch.randn(n, 16, generator=gen) * 3.0),
             ll_obs=_guarded(n, 235, torch.randn(n, 235, generator=gen) * 1.5))
    return types.SimpleNamespace(**t)


def _separate(pred, prey, ll, P, x, n, step, ctr, det_pred=False, det_prey=False):
    """``lg_lstm_actor_act`` x 2 -> ``lg_dec_game_pre`` on copies of the samples, and ``lg_policy_act(ll, deterministic = 1)``."""
    from legged_games_gym_amd import capi
    lib = capi.load_library()
    sp, mp, sy, my, act = _guarded(n, 2), _guarded(n, 2), _guarded(n, 4), _guarded(n, 4), _guarded(n, 12)
    assert lib.lg_lstm_actor_act(pred.handle, x.h_pred.data_ptr(), sp.data_ptr(), mp.data_ptr(), n, SEED_PRED, step, ctr, int(det_pred), _stream()) == 0
    assert lib.lg_lstm_actor_act(prey.handle, x.h_prey.data_ptr(), sy.data_ptr(), my.data_ptr(), n, SEED_PREY, step, ctr, int(det_prey), _stream()) == 0
    cp, cy, llc = sp[:n].clone(), sy[:n].clone(), torch.full((n, 4), 7.0, device=DEV)
    capi.dec_game_pre(P, capi.dec_game_buffers({"command_prey": cy.data_ptr(), "command_pred": cp.data_ptr(), "ll_commands": llc.data_ptr()}), _stream())
    assert lib.lg_policy_act(ll.handle, x.ll_obs.data_ptr(), act.data_ptr(), None, n, SEED_PREY, step, ctr, 1, _stream()) == 0
    torch.cuda.synchronize()
    return dict(command_pred=cp, command_prey=cy, ll_commands=llc, mean_pred=mp[:n], mean_prey=my[:n], sample_pred=sp[:n], sample_prey=sy[:n], ll_actions=act[:n])


WIDTHS = dict(command_pred=2, command_prey=4, ll_commands=4, ll_actions=12, mean_pred=2, mean_prey=4)
OPTIONAL = dict(sample_pred=2, sigma_pred=2, log_prob_pred=0, obs_copy_pred=3, sample_prey=4, sigma_prey=4, log_prob_prey=0, obs_copy_prey=16)


def _one_launch(pred, prey, ll, P, x, n, step, ctr, det_pred=False, det_prey=False, optional=True, seeds=(SEED_PRED, SEED_PREY)):
    from legged_games_gym_amd import capi
    out = {k: _guarded(n, w) for k, w in WIDTHS.items()}
    o_pred = o_prey = None
    if optional:
        out.update({k: _guarded(n, w) for k, w in OPTIONAL.items()})
        o_pred, o_prey = capi.lg_dec_act_outputs(), capi.lg_dec_act_outputs()
        for o, who in ((o_pred, "pred"), (o_prey, "prey")):
            for field in ("sample", "sigma", "log_prob", "obs_copy"):
                setattr(o, field, out[f"{field}_{who}"].data_ptr())
    B = capi.dec_game_buffers({k: out[k].data_ptr() for k in ("command_prey", "command_pred", "ll_commands")})
    rc = capi.dec_game_lstm_act(pred.handle, prey.handle, ll.handle, P, B, x.h_pred.data_ptr(), x.h_prey.data_ptr(), x.pred_obs.data_ptr(), x.prey_obs.data_ptr(),
                                x.ll_obs.data_ptr(), out["ll_actions"].data_ptr(), out["mean_pred"].data_ptr(), out["mean_prey"].data_ptr(), seeds[0], seeds[1],
                                step, ctr, det_pred, det_prey, o_pred, o_prey, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    for name, t in out.items():
        assert bool(torch.isnan(t[n:]).all()), f"{name}: the guard rows behind row {n} were written"
    return {k: v[:n] for k, v in out.items()}


COMPARED = ("command_pred", "command_prey", "ll_commands", "mean_pred", "mean_prey", "sample_pred", "sample_prey", "ll_actions")


@pytest.mark.parametrize("counter_on_device", [False, True], ids=["host_step", "device_counter"])
@pytest.mark.parametrize("heading", [1, 0], ids=["heading", "no_heading"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("H,hidden", ACTORS, ids=ACTOR_IDS)
def test_actor_launch_is_bit_identical_to_the_separate_launches(H, hidden, n, heading, counter_on_device):
    from legged_games_gym_amd import capi
    assert capi.load_library().lg_mlp_wide_set_precision(-1) == 1                  # the default; an invalid mode only reads it
    ((pred_p, pred), (prey_p, prey)), (_, ll) = _agents(H, hidden), _ll()
    x = _inputs(n, H, seed=100 + n)
    p = dt.params(num_envs=n, heading_command=heading)
    P = pack_params(p)
    step_value = 77 + n
    counter = torch.tensor([step_value - 1], dtype=torch.int64, device=DEV)        # the kernels read counter + 1
    step, ctr = (-1, counter.data_ptr()) if counter_on_device else (step_value, None)
    want = _separate(pred, prey, ll, P, x, n, step, ctr)
    got = _one_launch(pred, prey, ll, P, x, n, step, ctr)
    for name in COMPARED:
        assert torch.equal(got[name], want[name]), (name, float((got[name] - want[name]).abs().max()))
    assert torch.equal(got["obs_copy_pred"], x.pred_obs[:n]) and torch.equal(got["obs_copy_prey"], x.prey_obs[:n])
    assert torch.equal(got["ll_commands"], got["command_prey"]) and int(counter[0]) == step_value - 1
    assert torch.equal(got["sigma_pred"], pred_p.std.expand(n, 2)) and torch.equal(got["sigma_prey"], prey_p.std.expand(n, 4))
    assert torch.equal(got["command_prey"][:, 3], got["sample_prey"][:, 3])
    for who in ("pred", "prey"):
        assert float((got[f"sample_{who}"] - got[f"mean_{who}"]).abs().max()) > 0.0
    if not heading:
        assert torch.equal(got["command_prey"][:, 2], got["sample_prey"][:, 2])

    # the optional outputs are optional; deterministic per agent: that agent's command is its clipped mean, the other still samples
    bare = _one_launch(pred, prey, ll, P, x, n, step, ctr, optional=False)
    for name in WIDTHS:
        assert torch.equal(bare[name], got[name]), name
    cy, cp, _ = dt.pre(p, got["mean_prey"].cpu().numpy(), got["mean_pred"].cpu().numpy())
    det = _one_launch(pred, prey, ll, P, x, n, step, ctr, det_pred=True)
    assert np.array_equal(det["command_pred"].cpu().numpy(), cp) and torch.equal(det["sample_pred"], got["mean_pred"])
    assert torch.equal(det["command_prey"], got["command_prey"]) and torch.equal(det["mean_pred"], got["mean_pred"])
    det = _one_launch(pred, prey, ll, P, x, n, step, ctr, det_prey=True)
    assert np.array_equal(det["command_prey"].cpu().numpy(), cy) and np.array_equal(det["ll_commands"].cpu().numpy(), cy)
    assert torch.equal(det["sample_prey"], got["mean_prey"]) and torch.equal(det["command_pred"], got["command_pred"])
    assert torch.equal(det["ll_actions"], got["ll_actions"])
    det_w = _separate(pred, prey, ll, P, x, n, step, ctr, det_prey=True)
    assert torch.equal(det["command_prey"], det_w["command_prey"])


# ----------------------------------------------------------------------------- 3. clip and wrap really exercised
@pytest.mark.parametrize("heading", [1, 0], ids=["heading", "no_heading"])
def test_clip_and_wrap_are_exercised_on_both_sides(heading):
    """n = 65 with the biases and stds above: every clipped column has samples outside and inside its range, the prey's column 2 samples
    beyond +-pi and inside -- asserted before what happened to them is."""
    H, hidden = ACTORS[1]
    n = 65
    ((_, pred), (_, prey)), (_, ll) = _agents(H, hidden), _ll()
    x = _inputs(n, H, seed=100 + n)
    p = dt.params(num_envs=n, heading_command=heading)
    got = _one_launch(pred, prey, ll, pack_params(p), x, n, 142, None)
    for who, col, hi in (("prey", 0, 1.0), ("prey", 1, 1.0), ("pred", 0, 2.0), ("pred", 1, 2.0)):
        sample, command = got[f"sample_{who}"], got[f"command_{who}"]
        out = sample[:, col].abs() > hi
        assert bool(out.any()) and bool((~out).any()), (who, col)
        assert bool((command[out][:, col].abs() == hi).all()) and torch.equal(command[~out][:, col], sample[~out][:, col]), (who, col)
        assert torch.equal(torch.sign(command[out][:, col]), torch.sign(sample[out][:, col])), (who, col)
    sample, command = got["sample_prey"], got["command_prey"]
    beyond = sample[:, 2].abs() > math.pi
    assert bool(beyond.any()) and bool((~beyond).any())
    if heading:
        assert bool((command[beyond][:, 2].abs() <= math.pi).all()) and not torch.equal(command[:, 2], sample[:, 2])
        turn = (sample[beyond][:, 2].double() - command[beyond][:, 2].double()) / (2.0 * math.pi)
        assert float((turn - turn.round()).abs().max()) < 1e-6                      # the same angle, a whole number of turns away
    else:
        assert torch.equal(command[:, 2], sample[:, 2])
    cy, cp, llc = dt.pre(p, sample.cpu().numpy(), got["sample_pred"].cpu().numpy())  # the NumPy twin of lg_dec_game_pre
    assert np.array_equal(command.cpu().numpy(), cy) and np.array_equal(got["command_pred"].cpu().numpy(), cp)
    assert np.array_equal(got["ll_commands"].cpu().numpy(), llc)


# ----------------------------------------------------------------------------- 4. against float64 outside any kernel
def test_actor_launch_matches_float64_forwards_and_log_probs():
    """n = 33 (a second workgroup per role) at the task's default actors: both means within 2e-5 of the output scale of ``actor_forward64``,
    the low-level actions within 1e-4 (the split-bf16 bar), both ``log_prob`` within 2e-5 of a float64 Normal log-prob of (``sample``,
    ``mean``, std): the three bars of tests/test_gpu_game_recurrent.py."""
    H, hidden = ACTORS[1]
    n = 33
    ((pred_p, pred), (prey_p, prey)), (ll_ac, ll) = _agents(H, hidden), _ll()
    x = _inputs(n, H, seed=133)
    got = _one_launch(pred, prey, ll, pack_params(dt.params(num_envs=n)), x, n, 110, None)
    for name, key, layers, inp, tol in (("predator mean", "mean_pred", pred_p.actor, x.h_pred[:n], 2e-5), ("prey mean", "mean_prey", prey_p.actor, x.h_prey[:n], 2e-5),
                                        ("low-level actions", "ll_actions", ll_ac.actor, x.ll_obs[:n], 1e-4)):
        want = actor_forward64(*actor_params64(layers), inp.cpu().double().numpy())
        err, scale = float(np.abs(got[key].cpu().double().numpy() - want).max()), max(1.0, float(np.abs(want).max()))
        print(f"[observed] k_dec_game_lstm_act n {n} {name}: err {err:.3e}, scale {scale:.3f}, err / scale {err / scale:.3e} (bar {tol:g})")
        assert err < tol * scale, (name, err, scale)
    for who, policy in (("pred", pred_p), ("prey", prey_p)):
        sample, mean, std = got[f"sample_{who}"].cpu().double(), got[f"mean_{who}"].cpu().double(), policy.std.cpu().double()
        z = (sample - mean) / std
        want_lp = (-0.5 * z * z - std.log() - 0.5 * math.log(2.0 * math.pi)).sum(-1)
        err = float((got[f"log_prob_{who}"].cpu().double() - want_lp).abs().max())
        print(f"[observed] k_dec_game_lstm_act n {n} log_prob {who}: err {err:.3e}, max |z| {float(z.abs().max()):.2f} (bar 2e-5)")
        assert err < 2e-5, (who, err)


# ----------------------------------------------------------------------------- 5. noise
def test_noise_is_the_reference_philox_stream_under_each_agents_seed():
    """``sample - mean`` of both agents is ``std * eps`` of the NumPy Philox reference for (the agent's seed; env, step), with the step from
    the host, beyond 2^32 and from a device counter holding step - 1; equal seeds are refused."""
    H, hidden = ACTORS[0]
    n = 37
    ((pred_p, pred), (prey_p, prey)), (_, ll) = _agents(H, hidden), _ll()
    x = _inputs(n, H, seed=6)
    P = pack_params(dt.params(num_envs=n))
    report = {}

    def check(got, step):
        for who, policy, seed in (("pred", pred_p, SEED_PRED), ("prey", prey_p, SEED_PREY)):
            check_noise(got[f"sample_{who}"].cpu().numpy(), got[f"mean_{who}"].cpu().numpy(), policy.std.cpu().double().numpy(), seed, step, report)

    for step in (41, 2 ** 32 + 4242):
        check(_one_launch(pred, prey, ll, P, x, n, step, None), step)
    c = 776
    counter = torch.tensor([c], dtype=torch.int64, device=DEV)
    got = _one_launch(pred, prey, ll, P, x, n, -1, counter.data_ptr())
    check(got, c + 1)
    assert int(counter[0]) == c
    by_host = _one_launch(pred, prey, ll, P, x, n, c + 1, None)
    assert torch.equal(by_host["sample_pred"], got["sample_pred"]) and torch.equal(by_host["sample_prey"], got["sample_prey"])
    zp, zy = (got["sample_pred"] - got["mean_pred"]) / pred_p.std, (got["sample_prey"] - got["mean_prey"]) / prey_p.std
    assert float((zy[:, :2] - zp).abs().mean()) > 0.5                               # different seeds: different noise
    with pytest.raises(RuntimeError, match="must differ"):
        _one_launch(pred, prey, ll, P, x, n, 41, None, seeds=(5, 5))
    print("[observed] k_dec_game_lstm_act noise: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(report.items())))


# ----------------------------------------------------------------------------- env fixtures
from tests.dec_game_fixtures import dec_registered  # noqa: E402,F401
from tests.test_gpu_dec_game import assert_same_state, make_dec  # noqa: E402
from tests.test_gpu_game import write_ll_checkpoint  # noqa: E402

N_ENV = 64


def _recurrent_policy(agent, units=64, hidden=(64, 64, 32), seed=6):
    from legged_games_gym_amd.rl import ActorCriticRecurrent
    no, na, bias, std = (16, 4, BIAS_PREY, STD_PREY) if agent == "prey" else (3, 2, BIAS_PRED, STD_PRED)
    torch.manual_seed(seed + no)
    ac = ActorCriticRecurrent(no, no, na, actor_hidden_dims=list(hidden), critic_hidden_dims=list(hidden), rnn_hidden_size=units).to(DEV)
    with torch.no_grad():
        ac.std.copy_(torch.tensor(std))
        ac.actor[-1].bias.copy_(torch.tensor(bias))
    return ac


def _policies():
    if "policies" not in _cache:
        _cache["policies"] = (_recurrent_policy("pred"), _recurrent_policy("prey"))
    return _cache["policies"]


def _pair(env=None, seeds=(21 + 104729, 21)):
    """Two ``RecurrentFusedActor`` s over the same two modules; on ``env``'s device step counter when given."""
    from legged_games_gym_amd.rl.recurrent_actor import RecurrentFusedActor
    ctr = None if env is None else env.ll_env._sim.buf["step_counter"]
    pred, prey = _policies()
    return (RecurrentFusedActor(pred, DEV, seed=seeds[0], step_counter=ctr, num_envs=N_ENV),
            RecurrentFusedActor(prey, DEV, seed=seeds[1], step_counter=ctr, num_envs=N_ENV))


def _two_envs(tmp_path, seed=9, reset_seed=90, outcome=(False, False)):
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)         # a random low-level policy
    A, B = make_dec(ckpt, N_ENV, seed=seed), make_dec(ckpt, N_ENV, seed=seed)
    for env, on in zip((A, B), outcome):
        if on:
            env.enable_outcome_stats()
        torch.manual_seed(reset_seed)                                              # reset_idx from the host draws from torch's generator
        env.reset()
        env.ll_env.episode_length_buf[::2] = int(env.ll_env.max_episode_length) - 2 - (torch.arange(0, N_ENV, 2, device=DEV) % 7)     # low-level time-outs within a few steps
    assert torch.equal(A.obs_buf_prey, B.obs_buf_prey) and torch.equal(A.ll_env.root_states, B.ll_env.root_states) and torch.equal(A.predator_pos, B.predator_pos)
    return A, B


def _same_memories(fa, fb):
    return all(torch.equal(x, y) for pa, pb in zip(fa.hidden_states(), fb.hidden_states()) for x, y in zip(pa, pb))


# ----------------------------------------------------------------------------- 6. the env
def test_step_policy_equals_its_pieces(tmp_path):
    """A: ``step_policy(RecurrentFusedActor, RecurrentFusedActor)``.  B, identically seeded: ``step_memories`` per agent ->
    ``lg_lstm_actor_act`` per agent -> ``env.step(commands)`` (``lg_dec_game_pre``, the low-level actor, ``lg_step``, the post kernel).  Six
    steps, every choice of critic memories, a reset forced in between; commands, means, samples, critic outputs, env state, observations and
    all four memories bit for bit."""
    A, B = _two_envs(tmp_path)
    (pa, ya), (pb, yb) = _pair(), _pair()
    forced = torch.arange(3, N_ENV, 5, device=DEV)
    sample_p, sample_y = torch.empty(N_ENV, 2, device=DEV), torch.empty(N_ENV, 4, device=DEV)
    critic_sets = [("pred",), ("prey",), (), ("pred", "prey"), (), ("pred",)]
    resets = 0
    for k, critics in enumerate(critic_sets):
        prev_pred, prev_prey, flags = A.obs_buf_pred, A.obs_buf_prey, B.reset_buf.clone()
        read_pred, read_prey = prev_pred.clone(), prev_prey.clone()
        pred_a, prey_a, res = A.step_policy(pa, ya, out_pred={"sample": sample_p}, out_prey={"sample": sample_y}, with_critic_memory=critics)
        hp, hcp = pb.step_memories(B.obs_buf_pred, B.obs_buf_pred if "pred" in critics else None, reset=B.reset_buf)
        hy, hcy = yb.step_memories(B.obs_buf_prey, B.obs_buf_prey if "prey" in critics else None, reset=B.reset_buf)
        act_p, mean_p = pb.fused.act_with_mean(hp)
        act_y, mean_y = yb.fused.act_with_mean(hy)
        raw_p, raw_y = act_p.clone(), act_y.clone()
        B.step(act_p, act_y)                                                       # clips where they are
        torch.cuda.synchronize()
        assert A.last_act_rc == 0, k
        assert len(pred_a) == (3 if "pred" in critics else 2) and len(prey_a) == (3 if "prey" in critics else 2), k
        assert torch.equal(pred_a[0], act_p) and torch.equal(prey_a[0], act_y) and torch.equal(pred_a[1], mean_p) and torch.equal(prey_a[1], mean_y), k
        assert torch.equal(sample_p, raw_p) and torch.equal(sample_y, raw_y), k
        if "pred" in critics:
            assert torch.equal(pred_a[2], hcp), k
        if "prey" in critics:
            assert torch.equal(prey_a[2], hcy), k
        assert res[1] is A.obs_buf_prey and res[1] is not prev_prey and res[0] is not prev_pred, k
        assert torch.equal(prev_prey, read_prey) and torch.equal(prev_pred, read_pred), k      # the observations the memories read stay where they were
        assert_same_state(A, B, k)
        assert _same_memories(pa, pb) and _same_memories(ya, yb), k
        assert pa._flip == pb._flip and ya._flip == yb._flip and pa.fused._host_step == pb.fused._host_step == k + 1
        assert A.ll_env.common_step_counter == B.ll_env.common_step_counter and A._obs_flip == B._obs_flip
        if k == 1:                                                                 # a reset row's memories started from zero
            from legged_games_gym_amd.rl.recurrent_actor import RecurrentFusedActor
            fresh = RecurrentFusedActor(_policies()[1], DEV, seed=21, num_envs=N_ENV)
            fresh.step_memories(read_prey, read_prey)
            rows, live = flags.nonzero().flatten(), (~flags).nonzero().flatten()
            assert set(forced.tolist()) <= set(rows.tolist()) and len(live) > 0
            for mine, zero in zip(ya.hidden_states(), fresh.hidden_states()):
                for x, y in zip(mine, zero):
                    assert torch.equal(x[0, rows], y[0, rows])
            assert not torch.equal(ya.hidden_states()[0][0][0, live], fresh.hidden_states()[0][0][0, live])
        resets += int(A.reset_buf.sum())
        for env in (A, B):                                                         # the reset forced in between
            env.reset_buf[forced] = True
    assert resets > 0
    assert float(pa.hidden_states()[1][0].abs().max()) > 0.0 and float(ya.hidden_states()[1][0].abs().max()) > 0.0
    # an opponent pool next to a recurrent actor, a mixed pair
    with pytest.raises(ValueError, match="pool is feed-forward"):
        A.step_policy(pa, types.SimpleNamespace(is_opponent_pool=True, live=types.SimpleNamespace()))
    with pytest.raises(ValueError, match="with_critic_memory"):
        A.step_policy(pa, ya, with_critic_memory=("predator",))
    assert A._obs_flip == B._obs_flip                                              # (a refused call leaves the ping-pong where it was)


@pytest.mark.parametrize("steps_per_replay", [1, 2])
def test_graphed_policy_step_equals_the_eager_one(tmp_path, steps_per_replay):
    """Memories from zero on the sims' device step counters: three warm-up steps and the capture on A, the same steps eagerly on B.  One step
    per replay holds the slots of both actors."""
    A, B = _two_envs(tmp_path)
    (pa, ya), (pb, yb) = _pair(A), _pair(B)
    with pytest.raises(ValueError):
        A.make_graphed_policy_step(*_pair())                                       # host-counted noise streams cannot be replayed
    assert A.shared_actor_launch(pa, ya) is True and not any(float(t.abs().max()) for f in (pa, ya) for pair in f.hidden_states() for t in pair)
    flips = (pa._flip, ya._flip)
    replay = A.make_graphed_policy_step(pa, ya, warmup=3, steps_per_replay=steps_per_replay)
    assert A.last_act_rc == 0
    for _ in range(3):
        B.step_policy(pb, yb)
    if steps_per_replay == 1:
        assert (pa._flip, ya._flip) == flips
    for k in range(4):
        replay()
        for _ in range(steps_per_replay):
            B.step_policy(pb, yb)
        torch.cuda.synchronize()
        for fa, fb in ((pa, pb), (ya, yb)):
            assert all(torch.equal(a, b) for a, b in zip(fa.output_buffers(N_ENV), fb.output_buffers(N_ENV))), k
            assert all(torch.equal(x, y) for x, y in zip(fa.hidden_states()[0], fb.hidden_states()[0])), k      # the actor memories
        assert_same_state(A, B, k)
        for env in (A, B):
            assert int(env.ll_env._sim.buf["step_counter"][0]) == env.ll_env.common_step_counter
    assert float(pa.hidden_states()[0][0].abs().max()) > 0.0 and float(ya.hidden_states()[0][0].abs().max()) > 0.0
    assert float(pa.hidden_states()[1][0].abs().max()) == 0.0                        # no critic memory was in the cell launch


def test_env_takes_the_separate_launches_at_precision_0_on_rc_minus_4_and_without_the_library(tmp_path, monkeypatch, capsys):
    from legged_games_gym_amd import capi
    lib = capi.load_library()
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    env = make_dec(ckpt, N_ENV, seed=9)
    env.reset()
    pf, yf = _pair()
    launches = []
    real = capi.dec_game_lstm_act
    monkeypatch.setattr(capi, "dec_game_lstm_act", lambda *a, **k: launches.append(real(*a, **k)) or launches[-1])
    obs_pred, obs_prey = env.obs_buf_pred, env.obs_buf_prey
    other_prey = env._obs_pair_prey[env._obs_flip ^ 1]

    def act():
        for f in (pf, yf):
            f.reset_states()
            f._flip, f.fused._host_step = 0, 0
        other_prey.fill_(float("nan"))
        out_p = dict(sample=torch.empty(N_ENV, 2, device=DEV), sigma=torch.empty(N_ENV, 2, device=DEV), log_prob=torch.empty(N_ENV, device=DEV))
        out_y = dict(sample=torch.empty(N_ENV, 4, device=DEV), sigma=torch.empty(N_ENV, 4, device=DEV), log_prob=torch.empty(N_ENV, device=DEV))
        (cp, mp), (cy, my), ll_actions, _ = env._act(pf, yf, obs_pred, obs_prey, env._obs_pair_pred[env._obs_flip ^ 1], other_prey, False, False, out_p, out_y,
                                                     with_critic_memory=("prey",))
        torch.cuda.synchronize()
        assert pf.fused._host_step == yf.fused._host_step == 1 and torch.equal(other_prey, obs_prey)
        exact = [cp, mp, cy, my, out_p["sample"], out_p["sigma"], out_y["sample"], out_y["sigma"], env.ll_env.commands, env._critic_out["prey"],
                 pf.hidden_states()[0][0], yf.hidden_states()[0][0]]
        assert env._critic_out["pred"] is None
        return [t.clone() for t in exact], [out_p["log_prob"].clone(), out_y["log_prob"].clone()], ll_actions.clone()

    capsys.readouterr()
    want = act()
    assert launches == [0] and capsys.readouterr().out == ""                        # the one launch, not a word
    del launches[:]

    def check(got, tag, same_ll):
        for i, (a, b) in enumerate(zip(got[0], want[0])):
            assert torch.equal(a, b), (tag, i)
        for a, b in zip(got[1], want[1]):
            assert float((a - b).abs().max()) < 2e-5, tag                           # (the log-prob of the separate launches is torch's)
        assert torch.equal(got[2], want[2]) == same_ll, tag

    old = lib.lg_mlp_wide_set_precision(0)
    try:
        got = act()
        out = capsys.readouterr().out
        assert launches == [] and out.count("\n") == 1 and "wide precision 0" in out and "lg_lstm_actor_act x 2" in out, out
        check(got, "precision 0", same_ll=False)                                   # (the low-level actor is then the exact-f32 kernel)
        assert env.shared_actor_launch(pf, yf) is False
        act()
        assert capsys.readouterr().out == ""                                       # said once
    finally:
        lib.lg_mlp_wide_set_precision(old)
    assert lib.lg_mlp_wide_set_precision(-1) == 1

    # rc -4: the library is handed the actors the other way round (a four-action predator, a two-action prey)
    monkeypatch.setattr(capi, "dec_game_lstm_act", lambda pred, prey, *a, **k: launches.append(real(prey, pred, *a, **k)) or launches[-1])
    got = act()
    out = capsys.readouterr().out
    assert launches == [-4] and out.count("\n") == 1 and "no kernel for this actor pair" in out, out
    check(got, "rc -4", same_ll=True)
    monkeypatch.setattr(capi, "dec_game_lstm_act", real)

    # without the library: lg_lstm_step per agent as well
    monkeypatch.setattr(capi.LIBRARIES["dec_game_recurrent"], "handle", None)
    monkeypatch.setenv("LG_DEC_GAME_RECURRENT_LIB", str(tmp_path / "absent.so"))
    got = act()
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "absent.so" in out and "lg_lstm_actor_act x 2" in out, out
    check(got, "no library", same_ll=True)


def test_outcome_statistics_change_nothing_and_count(tmp_path):
    A, B = _two_envs(tmp_path, outcome=(False, True))
    (pa, ya), (pb, yb) = _pair(), _pair()
    for k in range(10):
        A.step_policy(pa, ya, with_critic_memory=("prey",))
        B.step_policy(pb, yb, with_critic_memory=("prey",))
        torch.cuda.synchronize()
        assert A.last_act_rc == B.last_act_rc == 0
        assert_same_state(A, B, k)
        assert _same_memories(pa, pb) and _same_memories(ya, yb), k
    totals = B.outcome_totals()
    assert totals["episodes"] >= N_ENV // 2 and totals["ll_timed_out"] >= N_ENV // 2, totals
    assert any(k.startswith("outcome_") for k in B.extras["episode"]) and not any(k.startswith("outcome_") for k in A.extras["episode"])


# ----------------------------------------------------------------------------- 7. the runner
def _dec_runner(reg, tmp_path, monkeypatch, ckpt, n=N_ENV, units=64, **runner_keys):
    import legged_games_gym_amd.utils.task_registry as tr_mod
    from legged_games_gym_amd.utils import get_args
    from legged_games_gym_amd.utils.helpers import apply_policy_args
    monkeypatch.setattr(tr_mod, "LEGGED_GYM_ROOT_DIR", str(tmp_path))
    env_cfg, train_cfg = reg.get_cfgs("dec_high_level_game")
    env_cfg.env.ll_policy_path = ckpt
    for key in ("graphed_rollout",):
        if hasattr(train_cfg.runner, key):
            delattr(train_cfg.runner, key)
    train_cfg.runner.device_rollout = True                                  # a runner key, not a config field: set on this registration only
    for key, value in runner_keys.items():
        setattr(train_cfg.runner, key, value)
    args = get_args(["--task", "dec_high_level_game", "--num_envs", str(n), "--headless", "--sim_device", DEV, "--rl_device", DEV,
                     "--policy_class_name", "ActorCriticRecurrent", "--rnn_hidden_size", str(units)])
    apply_policy_args(train_cfg, args)
    env, _ = reg.make_env("dec_high_level_game", args)
    torch.manual_seed(1234)
    runner, _ = reg.make_dec_alg_runner(env, "dec_high_level_game", args)
    # episodes that end inside the first rollouts: low-level time-outs 3 .. 43 steps ahead on every other env
    env.ll_env.episode_length_buf[::2] = int(env.ll_env.max_episode_length) - 3 - (torch.arange(0, n, 2, device=DEV) % 41)
    return env, runner, args


def test_runner_trains_two_recurrent_policies_saves_loads_and_plays(tmp_path, monkeypatch, dec_registered, capsys):
    import json
    import os
    from legged_games_gym_amd.rl.recurrent_actor import RecurrentFusedActor
    from legged_games_gym_amd.scripts import play_dec_game as pdg
    from tests.test_gpu_game_recurrent import _check_storage_against_batch_mode, _stats
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    try:
        env, runner, _ = _dec_runner(dec_registered, tmp_path, monkeypatch, ckpt)
        assert runner.recurrent and runner.device_path
        for a, other in (("pred", "prey"), ("prey", "pred")):
            r = runner.runners[a]
            assert isinstance(r._fused, RecurrentFusedActor) and r._game_rollout and r._recurrent_rollout
            assert runner.views[a].opponent is runner.runners[other]._fused
            assert r.alg.actor_critic.memory_a.rnn.hidden_size == 64
        T = runner.runners["pred"].num_steps_per_env

        # a rollout of each view against the torch module in batch mode over the stored observations and initial hidden states
        for a in ("pred", "prey"):
            r = runner.runners[a]
            with torch.inference_mode():
                r._rollout_steps(_stats(r))
                torch.cuda.synchronize()
                if a == "prey":                                                    # a carried-in state: its actor memory moved as the predator's opponent
                    assert float(r.alg.storage.initial_hidden_a[0].abs().max()) > 0.0 and float(r.alg.storage.initial_hidden_c[0].abs().max()) == 0.0
                _check_storage_against_batch_mode(r, f"dec {a} view, eager rollout")
            r.alg.storage.clear()

        params = lambda a: [p.detach().clone() for p in runner.runners[a].alg.actor_critic.parameters()]
        before = {a: params(a) for a in ("pred", "prey")}
        # the agent that becomes the learner starts its evolution with a zero critic state in both slots
        seen = {}
        for a in ("pred", "prey"):
            r = runner.runners[a]
            for pair in r._fused.state_c:
                for t in pair:
                    t.fill_(0.5)
            r._fused._critic_slots_equal = False

            def learn(*x, _r=r, _a=a, _learn=r.learn, **k):
                seen[_a] = max(float(t.abs().max()) for pair in _r._fused.state_c for t in pair)
                return _learn(*x, **k)
            r.learn = learn
        actor_state = float(runner.runners["prey"]._fused.hidden_states()[0][0].abs().max())
        assert actor_state > 0.0
        runner.learn(max_num_evolutions=1, num_learning_iterations=2)
        torch.cuda.synchronize()
        assert seen == {"pred": 0.0}
        assert all(torch.equal(x, y) for x, y in zip(before["prey"], params("prey")))          # the opponent is not updated ...
        assert any(not torch.equal(x, y) for x, y in zip(before["pred"], params("pred")))      # ... the learner is, memories included
        ac = runner.runners["pred"].alg.actor_critic
        assert not torch.equal(before["pred"][[n for n, _ in ac.named_parameters()].index("memory_a.rnn.weight_hh_l0")], ac.memory_a.rnn.weight_hh_l0)
        assert max(float(t.abs().max()) for pair in runner.runners["prey"]._fused.state_c for t in pair) == 0.5      # the opponent's critic memory rested
        assert float(runner.runners["prey"]._fused.hidden_states()[0][0].abs().max()) > 0.0                        # ... its actor memory carried on
        mid = params("pred")
        runner.learn(max_num_evolutions=1, num_learning_iterations=2)
        torch.cuda.synchronize()
        assert seen == {"pred": 0.0, "prey": 0.0} and runner.current_evolution == 2 and runner.current_learning_iteration == 4
        assert all(torch.equal(x, y) for x, y in zip(mid, params("pred"))) and any(not torch.equal(x, y) for x, y in zip(before["prey"], params("prey")))
        assert all(bool(torch.isfinite(p).all()) for a in ("pred", "prey") for p in runner.runners[a].alg.actor_critic.parameters())
        said = capsys.readouterr().out
        with capsys.disabled():
            print("".join(line + "\n" for line in said.splitlines() if line.startswith("[")))
        assert "unavailable" not in said

        # save -> load
        path = os.path.join(runner.log_dir, "model_4.pt")
        assert os.path.isfile(path)
        d = torch.load(path, map_location="cpu", weights_only=True)
        assert set(d) == {"pred", "prey", "evolution", "iter"} and d["evolution"] == 2 and d["iter"] == 4
        for a in ("pred", "prey"):
            keys = set(d[a]["model_state_dict"])
            assert {"memory_a.rnn.weight_ih_l0", "memory_a.rnn.weight_hh_l0", "memory_c.rnn.bias_ih_l0", "memory_c.rnn.bias_hh_l0"} <= keys
        after = {a: params(a) for a in ("pred", "prey")}
        with torch.no_grad():
            for a in ("pred", "prey"):
                for p in runner.runners[a].alg.actor_critic.parameters():
                    p.add_(1.0)
        runner.load(path)
        assert all(torch.equal(x, y) for a in ("pred", "prey") for x, y in zip(after[a], params(a))) and runner.current_evolution == 2

        # play_dec_game --outcomes on the checkpoint: the graphed policy step, both agents deterministic, memories from zero
        args = pdg._args(["--task", "dec_high_level_game", "--num_envs", "32", "--steps", "12", "--outcomes", "--headless", "--sim_device", DEV, "--rl_device", DEV,
                          "--policy_class_name", "ActorCriticRecurrent", "--rnn_hidden_size", "64", "--load_run", os.path.basename(runner.log_dir)])
        env_p, result, out = pdg.play_outcomes(args, steps=args.steps)
        assert out == os.path.join(runner.log_dir, "outcomes_4.json") and json.load(open(out)) == json.loads(json.dumps(result))
        assert result["path"] == "graphed policy step" and result["iteration"] == 4 and result["steps"] == 12 and result["num_envs"] == 32
        assert torch.isfinite(env_p.obs_buf_prey).all() and torch.isfinite(env_p.obs_buf_pred).all()
    finally:
        _, train_cfg = dec_registered.get_cfgs("dec_high_level_game")              # the registered object is shared: leave it as it was found
        for obj, keys in ((train_cfg.runner, ("device_rollout", "policy_class_name")), (train_cfg.policy, ("rnn_hidden_size",))):
            for key in keys:
                if key in vars(obj):
                    delattr(obj, key)
