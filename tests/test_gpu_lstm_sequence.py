"""-m gpu: the LSTM sequence kernels of the recurrent update (``lg_lstm_seq_forward`` / ``lg_lstm_seq_backward``,
include/legged_lstm_sequence.h) and what sits on them (``rl.lstm_sequence``, ``Memory.sequence``, ``PPO(device_bptt=True)``, the runner key).

Reference: a ``.double()`` copy of the ``nn.LSTM`` on the CPU, stepped through time so that every ``c_t`` is seen, with autograd in float64
(one small case also against ``tests/recurrent_ref.lstm_step64``).  Bars, the project's own: outputs within ``TOL = 2e-5`` of
``max(1, max |want|)`` (tests/test_gpu_recurrent.py), gradients through ``wide_learner_check.compare`` with ``rel = GRAD_TOL[0] = 1e-4`` of
``max |want|`` and ``GRAD_ABS``.  Control, in every case: float32 torch autograd on the same inputs is within a quarter of each bar, so the
bars are about the kernels and not about float32.

Inputs: trajectory lengths in 1 .. T (trajectory 0 full), ``x`` and ``dh_out`` zero beyond each length (what ``split_and_pad_trajectories``
and ``unpad_trajectories``' backward produce), ``h0`` / ``c0`` non-zero: the recipe of tests/lstm_seq_check.make_inputs, which
tests/test_gpu_lstm_sequence_edges.py runs at the kernels' shape edges.  The float64 references are computed once per case and shared."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import lstm_seq_check as lc
from tests.recurrent_ref import lstm_params64, lstm_step64
from tests.wide_learner_check import GRAD_ABS, GRAD_TOL, compare

pytestmark = pytest.mark.gpu
TOL = 2e-5
DEV = "cuda:0"
# (T, B, I, H): the smallest at which each mechanism can go wrong -- one of everything | odd K = 51 and one row past a block | 2 waves |
# the update's T | an exact block and 8 waves | the rough task's K = 491 (odd) | the largest LDS blocks, three workgroups
SHAPES = list(lc.OLD_SHAPES)
MID = (24, 37, 48, 64)
PARAMS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _reference(rnn, x, h0, c0, dh, dtype):
    """``nn.LSTM`` of ``dtype`` on the CPU, one step per call: (h [T, B, H], c [T, B, H], gradients of the four parameters)."""
    net = copy.deepcopy(rnn).to(dtype)
    h, c = h0.to(dtype).unsqueeze(0), c0.to(dtype).unsqueeze(0)
    hs, cs = [], []
    for t in range(x.shape[0]):
        out, (h, c) = net(x[t:t + 1].to(dtype), (h, c))
        hs.append(out[0])
        cs.append(c[0])
    hs, cs = torch.stack(hs), torch.stack(cs)
    (hs * dh.to(dtype)).sum().backward()
    return hs.detach(), cs.detach(), [getattr(net, n).grad.clone() for n in PARAMS]


@functools.lru_cache(maxsize=None)
def _case(shape, scale=1.0, saturate=False):
    """Inputs, the float64 reference and the float32 control of one case (all on the CPU; never modified afterwards)."""
    rnn, x, h0, c0, dh, lengths = lc.make_inputs(shape, scale, saturate)
    want = _reference(rnn, x, h0, c0, dh, torch.float64)
    ctrl = _reference(rnn, x, h0, c0, dh, torch.float32)
    # the control: float32 torch is within a quarter of every bar
    for name, got, ref in (("h", ctrl[0], want[0]), ("c", ctrl[1], want[1])):
        err, s = float((got.double() - ref).abs().max()), max(1.0, float(ref.abs().max()))
        assert err < 0.25 * TOL * s, f"control {shape} {name}: float32 torch is {err:.3e} from float64"
    for name, got, ref in zip(PARAMS, ctrl[2], want[2]):
        compare(f"control {shape} {name}.grad", got, ref, rel=0.25 * GRAD_TOL[0], abs_tol=0.25 * GRAD_ABS)
    return dict(shape=shape, rnn=rnn, x=x, h0=h0, c0=c0, dh=dh, lengths=lengths, want_h=want[0], want_c=want[1], want_grads=want[2])


def _lib():
    from legged_games_gym_amd import capi
    return capi.load_lstm_seq_library()


def _guarded(n, guard=257):
    """A NaN-filled float buffer of ``n`` elements with ``guard`` NaN elements behind it: (whole, view of the first n)."""
    whole = torch.full((n + guard,), float("nan"), device=DEV)
    return whole, whole[:n]


def _handle(lib, rnn_dev):
    h = C.c_void_p()
    assert lib.lg_lstm_seq_create(rnn_dev.input_size, rnn_dev.hidden_size, 0, C.byref(h)) == 0, lib.lg_lstm_seq_last_error()
    ps = [getattr(rnn_dev, n) for n in PARAMS]
    assert lib.lg_lstm_seq_load_device(h, *[p.data_ptr() for p in ps], _stream()) == 0, lib.lg_lstm_seq_last_error()
    return h


def _forward(case, with_ws=True, strided=False):
    """``lg_lstm_seq_forward`` on the case's inputs: (h_out [T, B, H], ws or None, the guarded wholes, device inputs, handle, rnn)."""
    T, B, I, H = case["shape"]
    lib = _lib()
    rnn = copy.deepcopy(case["rnn"]).to(DEV)
    handle = _handle(lib, rnn)
    if strided:                                               # a slice [:, 3:3 + B] of a wider tensor whose other rows are NaN
        wide = torch.full((T, B + 5, I), float("nan"), device=DEV)
        wide[:, 3:3 + B] = case["x"].to(DEV)
        x = wide[:, 3:3 + B]
        assert not x.is_contiguous() or T == 1
    else:
        x = case["x"].to(DEV)
    h0, c0 = case["h0"].to(DEV), case["c0"].to(DEV)
    h_whole, h_out = _guarded(T * B * H)
    ws_whole, ws = _guarded(5 * T * B * H) if with_ws else (None, None)
    assert lib.lg_lstm_seq_workspace_floats(T, B, H) == 5 * T * B * H
    rc = lib.lg_lstm_seq_forward(handle, x.data_ptr(), x.stride(0) if T > 1 else B * I, h0.data_ptr(), c0.data_ptr(), h_out.data_ptr(),
                                 ws.data_ptr() if with_ws else None, T, B, _stream())
    assert rc == 0, lib.lg_lstm_seq_last_error()
    torch.cuda.synchronize()
    return dict(h_out=h_out.view(T, B, H), ws=ws, h_whole=h_whole, ws_whole=ws_whole, x=x, h0=h0, c0=c0, handle=handle, rnn=rnn, lib=lib)


def _check_forward(case, run, tag):
    T, B, I, H = case["shape"]
    s_h, s_c = max(1.0, float(case["want_h"].abs().max())), max(1.0, float(case["want_c"].abs().max()))
    e_h = float((run["h_out"].cpu().double() - case["want_h"]).abs().max())
    print(f"{tag} {case['shape']}: h err {e_h:.3e} (scale {s_h:.2f})", end="")
    assert torch.isfinite(run["h_out"]).all() and e_h < TOL * s_h, (tag, e_h)
    if run["ws"] is not None:
        c = run["ws"][4 * T * B * H:].view(T, B, H)
        e_c = float((c.cpu().double() - case["want_c"]).abs().max())
        print(f"  c err {e_c:.3e} (scale {s_c:.2f})", end="")
        assert torch.isfinite(run["ws"]).all() and e_c < TOL * s_c, (tag, e_c)
    print()


# ---------------------------------------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_matches_float64_with_and_without_a_workspace(shape):
    case = _case(shape)
    run = _forward(case)
    _check_forward(case, run, "forward")
    bare = _forward(case, with_ws=False)
    assert torch.equal(bare["h_out"], run["h_out"]), "ws == NULL changes h_out"
    assert torch.isnan(run["h_whole"][run["h_out"].numel():]).all() and torch.isnan(run["ws_whole"][run["ws"].numel():]).all()
    for r in (run, bare):
        assert r["lib"].lg_lstm_seq_destroy(r["handle"]) == 0


def test_forward_with_weights_times_three_matches_float64():
    case = _case(MID, scale=3.0)
    _check_forward(case, _forward(case), "weights x 3")


@pytest.mark.parametrize("shape", [(2, 33, 19, 32), MID])
def test_forward_through_a_strided_input_equals_the_contiguous_one(shape):
    case = _case(shape)
    run = _forward(case, strided=True)
    _check_forward(case, run, "strided x")
    assert torch.equal(run["h_out"], _forward(case)["h_out"])


def test_forward_matches_the_explicit_float64_restatement():
    """``recurrent_ref.lstm_step64`` stepped through time: a reference that shares nothing with ``nn.LSTM``."""
    case = _case((3, 5, 17, 64))
    T = case["shape"][0]
    p64 = lstm_params64(case["rnn"])
    h, c = case["h0"].double().numpy(), case["c0"].double().numpy()
    hs = []
    for t in range(T):
        h, c = lstm_step64(p64, case["x"][t].numpy(), h, c)
        hs.append(h)
    got = _forward(case)["h_out"].cpu().double().numpy()
    err = np.abs(got - np.stack(hs)).max()
    print(f"against lstm_step64: {err:.3e}")
    assert err < TOL


# ---------------------------------------------------------------------------------------------------------------- 2. the rollout's cell
def _check_against_the_stepped_cell(case):
    from legged_games_gym_amd.rl.recurrent_actor import DeviceLstm, lstm_step
    from legged_games_gym_amd import capi
    shape = case["shape"]
    T, B, I, H = shape
    run = _forward(case)
    cell, lib = DeviceLstm(run["rnn"], DEV), capi.load_library()
    h, c = run["h0"].clone(), run["c0"].clone()
    hs = []
    for t in range(T):
        h2, c2 = torch.empty_like(h), torch.empty_like(c)
        lstm_step(lib, cell, None, run["x"][t].contiguous(), None, None, (h, c), (h2, c2), None, None, B, _stream())
        h, c = h2, c2
        hs.append(h)
    torch.cuda.synchronize()
    hs = torch.stack(hs)
    err, scale = float((hs.double() - run["h_out"].double()).abs().max()), max(1.0, float(hs.abs().max()))
    c_last = run["ws"][4 * T * B * H:].view(T, B, H)[-1]
    print(f"{shape}: sequence against the stepped cell: err {err:.3e}; bit-equal h {torch.equal(hs, run['h_out'])}, last c {torch.equal(c, c_last)}")
    assert err < TOL * scale


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_matches_the_rollout_cell_stepped_through_time(shape):
    """T launches of ``lg_lstm_step`` (actor role only) from the same (h0, c0): the update's first epoch evaluates the policy that acted,
    so its probability ratio is 1 to the extent these two agree."""
    _check_against_the_stepped_cell(_case(shape))


# ---------------------------------------------------------------------------------------------------------------- 3. backward
def _autograd(case):
    """Forward + backward through ``DeviceLstmSequence``: (out, the four gradients, the module on the device)."""
    from legged_games_gym_amd.rl.lstm_sequence import DeviceLstmSequence
    rnn = copy.deepcopy(case["rnn"]).to(DEV)
    seq = DeviceLstmSequence(rnn, DEV)
    out = seq(case["x"].to(DEV), (case["h0"].to(DEV).unsqueeze(0), case["c0"].to(DEV).unsqueeze(0)))
    assert out.requires_grad
    out.backward(case["dh"].to(DEV))
    torch.cuda.synchronize()
    return out.detach(), [getattr(rnn, n).grad for n in PARAMS], rnn


def _check_backward(case, tag):
    out, grads, _ = _autograd(case)
    s_h = max(1.0, float(case["want_h"].abs().max()))
    assert float((out.cpu().double() - case["want_h"]).abs().max()) < TOL * s_h
    for name, got, want in zip(PARAMS, grads, case["want_grads"]):
        fig = compare(f"{tag} {case['shape']} {name}.grad", got, want, rel=GRAD_TOL[0], abs_tol=GRAD_ABS)
        print(f"{tag} {case['shape']} {name}.grad: {fig:.3e} of max |want| {float(want.abs().max()):.3e}")
    assert torch.equal(grads[2], grads[3]), "db_ih != db_hh"
    return out, grads


@pytest.mark.parametrize("shape", SHAPES)
def test_backward_matches_float64_autograd(shape):
    _check_backward(_case(shape), "backward")


def test_backward_with_weights_times_three_matches_float64_autograd():
    _check_backward(_case(MID, scale=3.0), "backward, weights x 3")


def test_no_grad_forward_keeps_no_workspace_and_equals_the_recorded_one():
    from legged_games_gym_amd.rl.lstm_sequence import DeviceLstmSequence
    case = _case((3, 5, 17, 64))
    rnn = copy.deepcopy(case["rnn"]).to(DEV)
    seq = DeviceLstmSequence(rnn, DEV)
    args = case["x"].to(DEV), (case["h0"].to(DEV).unsqueeze(0), case["c0"].to(DEV).unsqueeze(0))
    with torch.no_grad():
        bare = seq(*args)
    assert not bare.requires_grad and torch.equal(bare, seq(*args).detach())
    want = rnn(*args)[0].detach()
    assert float((bare - want).abs().max()) < TOL


# ---------------------------------------------------------------------------------------------------------------- 4. saturated gates
def test_saturated_gates_stay_finite_and_within_the_bars():
    """Pre-activations of +-30, +-100 and +-1e4 in every gate: s (1 - s) and 1 - tanh^2 come out exactly 0, not NaN through inf . 0."""
    case = _case(MID, saturate=True)
    _check_forward(case, _forward(case), "saturated")
    out, grads = _check_backward(case, "saturated")
    assert all(bool(torch.isfinite(g).all()) for g in grads) and bool(torch.isfinite(out).all())
    assert float(case["want_grads"][0].abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------------------------- 5. / 6. bounds, determinism
def _forward_backward_raw(case):
    """Raw entry points with guards behind every buffer, inputs included: (outputs, guards as a list of (name, tensor))."""
    T, B, I, H = case["shape"]
    run = _forward(case)
    lib = run["lib"]
    gates_fwd = run["ws"][:4 * T * B * H].clone()
    padded = {}
    for name, src in (("dh", case["dh"]), ("w_hh", run["rnn"].weight_hh_l0.detach()), ("c0", case["c0"])):
        whole, view = _guarded(src.numel())
        view.copy_(src.reshape(-1))
        padded[name] = (whole, view)
    rc = lib.lg_lstm_seq_backward(run["handle"], padded["w_hh"][1].data_ptr(), padded["dh"][1].data_ptr(), padded["c0"][1].data_ptr(),
                                  run["ws"].data_ptr(), T, B, _stream())
    assert rc == 0, lib.lg_lstm_seq_last_error()
    torch.cuda.synchronize()
    guards = [("h_out", run["h_whole"][T * B * H:]), ("ws", run["ws_whole"][5 * T * B * H:])] + [(n, w[v.numel():]) for n, (w, v) in padded.items()]
    return run, gates_fwd, guards


@pytest.mark.parametrize("shape", [(2, 33, 19, 32), (3, 5, 17, 64), (24, 32, 48, 256), (5, 64, 235, 256)])
def test_outputs_are_written_everywhere_and_nothing_behind_them(shape):
    case = _case(shape)
    T, B, I, H = shape
    run, gates_fwd, guards = _forward_backward_raw(case)
    assert torch.isfinite(run["h_out"]).all() and torch.isfinite(run["ws"]).all() and torch.isfinite(gates_fwd).all()
    for name, g in guards:
        assert g.numel() > 0 and torch.isnan(g).all(), f"the guard behind {name} was written"
    # the gate block held gates after the forward and holds dG after the backward: db is its column sum
    assert float(gates_fwd.min()) >= -1.0 and float(gates_fwd.max()) <= 1.0
    db = run["ws"][:4 * T * B * H].view(T * B, 4 * H).double().sum(0).cpu()
    compare(f"{shape} column sums of dG", db, case["want_grads"][2], rel=GRAD_TOL[0], abs_tol=GRAD_ABS)


def test_forward_and_backward_are_bit_identical_from_run_to_run():
    case = _case((24, 96, 256, 256))
    (a, ga, _), (b, gb, _) = _forward_backward_raw(case), _forward_backward_raw(case)
    assert torch.equal(a["h_out"], b["h_out"]) and torch.equal(a["ws"], b["ws"]) and torch.equal(ga, gb)
    g1, g2 = _autograd(case)[1], _autograd(case)[1]
    assert all(torch.equal(x, y) for x, y in zip(g1, g2))


# ---------------------------------------------------------------------------------------------------------------- 7. through the module
def test_module_with_sequence_attached_matches_float64_in_every_parameter_gradient():
    from legged_games_gym_amd.rl.actor_critic import ActorCriticRecurrent
    from legged_games_gym_amd.rl.lstm_sequence import DeviceLstmSequence
    from legged_games_gym_amd.rl.ppo import RolloutStorage
    torch.manual_seed(5)
    T, N, O, A = 8, 6, 7, 3
    ac = ActorCriticRecurrent(O, O, A, [32, 32, 32], [32, 32, 32], rnn_hidden_size=32).to(DEV)
    ac64 = copy.deepcopy(ac).double().cpu()
    st = RolloutStorage(N, T, [O], [None], [A], DEV)
    gen = torch.Generator().manual_seed(11)
    st.observations.copy_(torch.rand(T, N, O, generator=gen) * 4 - 2)
    dones = torch.zeros(T, N, 1, dtype=torch.uint8)
    dones[2, 1] = dones[0, 2] = dones[5, 2] = dones[3, 4] = dones[4, 4] = dones[1, 5] = dones[7, 5] = 1      # envs with 1, 2 and 3 trajectories
    st.dones.copy_(dones)
    st.save_initial_hidden_states([tuple(torch.rand(1, N, 32, generator=gen) - 0.5 for _ in range(2)) for _ in range(2)])
    ac.memory_a.sequence, ac.memory_c.sequence = DeviceLstmSequence(ac.memory_a.rnn, DEV), DeviceLstmSequence(ac.memory_c.rnn, DEV)
    assert all("sequence" not in k for k in ac.state_dict()) and list(ac.state_dict()) == list(ac64.state_dict())
    batches = list(st.recurrent_mini_batch_generator(2, 1))
    assert len(batches) == 2 and sorted(b[0].shape[1] for b in batches) == [6, 6]           # 12 trajectories: 1 + 2 + 3 and 1 + 3 + 2 (a done at the last step ends nothing early)
    for n, (obs, cobs, act, val, adv, ret, lp, mu, sig, (hid_a, hid_c), masks) in enumerate(batches):
        R1 = torch.randn(T, N // 2, A, generator=gen)
        R2 = torch.randn(T, N // 2, 1, generator=gen)
        to64 = lambda t: t.detach().cpu().double()
        ac64.zero_grad()
        ac64.act(to64(obs), masks=masks.cpu(), hidden_states=tuple(to64(h) for h in hid_a))
        want_mu = ac64.action_mean
        want_val = ac64.evaluate(to64(cobs), masks=masks.cpu(), hidden_states=tuple(to64(h) for h in hid_c))
        ((want_mu * R1.double()).sum() + (want_val * R2.double()).sum()).backward()
        ac.zero_grad()
        ac.act(obs, masks=masks, hidden_states=hid_a)
        got_mu = ac.action_mean
        got_val = ac.evaluate(cobs, masks=masks, hidden_states=hid_c)
        ((got_mu * R1.to(DEV)).sum() + (got_val * R2.to(DEV)).sum()).backward()
        for name, got, want in (("mean", got_mu, want_mu), ("value", got_val, want_val)):
            err, s = float((got.detach().cpu().double() - want.detach()).abs().max()), max(1.0, float(want.detach().abs().max()))
            print(f"batch {n} {name}: err {err:.3e} (scale {s:.2f})")
            assert err < TOL * s, (name, err)
        grads64 = dict((k, p.grad) for k, p in ac64.named_parameters())
        for k, p in ac.named_parameters():
            if grads64[k] is None:                            # std: not on the path of the mean or the value
                assert p.grad is None, k
                continue
            fig = compare(f"batch {n} {k}.grad", p.grad, grads64[k], rel=GRAD_TOL[0], abs_tol=GRAD_ABS)
            print(f"batch {n} {k}.grad: {fig:.3e} of max")


# ---------------------------------------------------------------------------------------------------------------- 8. runner
def _runner(monkeypatch, hidden=64, **runner_keys):
    """``tests/test_gpu_recurrent._runner``: anymal_c_flat, 64 envs, 8 steps per rollout, every other env a few steps from a time-out."""
    from legged_games_gym_amd.envs import task_registry
    from legged_games_gym_amd.utils import get_args
    from legged_games_gym_amd.utils.helpers import apply_policy_args
    _, train_cfg = task_registry.get_cfgs("anymal_c_flat")
    args = get_args(["--task", "anymal_c_flat", "--num_envs", "64", "--headless", "--sim_device", DEV, "--rl_device", DEV,
                     "--policy_class_name", "ActorCriticRecurrent", "--rnn_hidden_size", str(hidden)])
    for obj, name in ((train_cfg.runner, "policy_class_name"), (train_cfg.runner, "num_steps_per_env"), (train_cfg.runner, "max_iterations"),
                      (train_cfg.policy, "rnn_hidden_size")):      # the registered cfg is shared: put every field back afterwards
        monkeypatch.setattr(obj, name, getattr(obj, name, None), raising=False)
    train_cfg.runner.num_steps_per_env = 8
    apply_policy_args(train_cfg, args)
    for name, value in runner_keys.items():
        monkeypatch.setattr(train_cfg.runner, name, value, raising=False)
    env, _ = task_registry.make_env("anymal_c_flat", args)
    runner, _ = task_registry.make_alg_runner(env, "anymal_c_flat", args, log_root=None)
    n = env.num_envs
    env.episode_length_buf[::2] = int(env.max_episode_length) - 2 - (torch.arange(0, n, 2, device=env.device) % 11)
    return env, runner


def _first_minibatch_grads(alg):
    ac = alg.actor_critic
    obs, cobs, act, tval, adv, ret, old_lp, old_mu, old_sig, hid, masks = next(iter(alg.storage.recurrent_mini_batch_generator(alg.num_mini_batches, 1)))
    ac.act(obs, masks=masks, hidden_states=hid[0])
    lp = ac.get_actions_log_prob(act)
    val = ac.evaluate(cobs, masks=masks, hidden_states=hid[1])
    loss, _, _ = alg._loss(lp, old_lp.squeeze(-1), adv.squeeze(-1), val, tval, ret, ac.entropy)
    ac.zero_grad()
    loss.backward()
    torch.cuda.synchronize()
    return {k: p.grad.clone() for k, p in ac.named_parameters()}


def test_runner_with_device_bptt_attaches_trains_and_agrees_with_torch(monkeypatch, capsys):
    from legged_games_gym_amd.rl.lstm_sequence import DeviceLstmSequence
    env, runner = _runner(monkeypatch, device_bptt=True)
    ac, alg = runner.alg.actor_critic, runner.alg
    assert isinstance(ac.memory_a.sequence, DeviceLstmSequence) and isinstance(ac.memory_c.sequence, DeviceLstmSequence)
    assert "unavailable" not in capsys.readouterr().out
    stats = {"cur_rew": torch.zeros(64, device=DEV), "cur_len": torch.zeros(64, device=DEV)}
    sums = torch.zeros(3, device=DEV)
    stats.update(sum_rew=sums[0], sum_len=sums[1], count=sums[2], _sums=sums)
    with torch.inference_mode():
        runner._rollout_steps(stats)
    torch.cuda.synchronize()
    assert int(alg.storage.dones.sum()) > 0, "no episode ended in the rollout: no second trajectory in the update"
    alg.storage.advantages.copy_(torch.randn(alg.storage.advantages.shape, generator=torch.Generator().manual_seed(3)))
    alg.storage.returns.copy_(alg.storage.values + 0.3 * torch.randn(alg.storage.values.shape, generator=torch.Generator().manual_seed(4)).to(DEV))
    on = _first_minibatch_grads(alg)
    kept = ac.memory_a.sequence, ac.memory_c.sequence
    ac.memory_a.sequence = ac.memory_c.sequence = None
    off = _first_minibatch_grads(alg)
    ac.memory_a.sequence, ac.memory_c.sequence = kept
    for k in on:
        fig = compare(f"{k}.grad, sequence on against torch", on[k], off[k], rel=GRAD_TOL[0], abs_tol=GRAD_ABS)
        print(f"{k}.grad: {fig:.3e} of max |torch| {float(off[k].abs().max()):.3e}")
    alg.storage.clear()
    before = ac.memory_a.rnn.weight_hh_l0.clone(), ac.memory_c.rnn.weight_ih_l0.clone()
    losses, update = [], alg.update
    monkeypatch.setattr(alg, "update", lambda: losses.append(update()) or losses[-1])
    runner.learn(2)
    print("losses (value, surrogate):", losses)
    assert len(losses) == 2 and all(np.isfinite(v) for pair in losses for v in pair), losses
    assert all(bool(torch.isfinite(p).all()) for p in ac.parameters())
    assert not torch.equal(before[0], ac.memory_a.rnn.weight_hh_l0) and not torch.equal(before[1], ac.memory_c.rnn.weight_ih_l0)
    assert ac.memory_a.sequence is kept[0] and "device BPTT unavailable" not in capsys.readouterr().out


def test_runner_with_device_bptt_keeps_torch_for_512_units(monkeypatch, capsys):
    env, runner = _runner(monkeypatch, hidden=512, device_bptt=True)
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if "device BPTT unavailable" in l]
    assert len(lines) == 1 and "512" in lines[0], out
    ac = runner.alg.actor_critic
    assert ac.memory_a.sequence is None and ac.memory_c.sequence is None
    before = ac.memory_a.rnn.weight_hh_l0.clone()
    runner.learn(1)
    assert not torch.equal(before, ac.memory_a.rnn.weight_hh_l0)
