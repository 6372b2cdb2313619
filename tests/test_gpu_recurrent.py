"""The LSTM cell of the recurrent policy on the GPU (``lg_lstm_step``, include/legged_recurrent.h) against the float64 restatement of
``tests/recurrent_ref.py`` (also with saturated gates and with NaN / Inf in the stale state of reset rows), the ``RecurrentFusedActor``
against the torch module (the default policy of ``anymal_c_rough`` against a float64 copy), and the runner's device rollout against
batch-mode evaluation of what it stored.  Inputs uniform in [-3, 3] and torch's default initialisation: the float32 ``nn.LSTM`` itself stays
within 7.5e-7 of float64 there, so 2e-5 (the bar of ``tests/test_gpu_rl.py``) leaves room for the 1-ulp ``v_rcp`` / ``v_exp``."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from tests.recurrent_ref import lstm_params64, lstm_step64, saturating_bias

pytestmark = pytest.mark.gpu
TOL = 2e-5
DEV = "cuda:0"


def _rnn(I, H, seed):
    torch.manual_seed(seed)
    return nn.LSTM(I, H).to(DEV)


def _uniform(gen, *shape):
    return (torch.rand(*shape, generator=gen) * 6.0 - 3.0).to(DEV)


def _padded(n, H, extra=5):
    """An output buffer of ``n`` rows with NaN sentinels behind it."""
    t = torch.full((n + extra, H), float("nan"), device=DEV)
    return t, t[:n]


def _cells():
    from legged_games_gym_amd.rl.recurrent_actor import DeviceLstm, lstm_step
    from legged_games_gym_amd import capi
    return DeviceLstm, lstm_step, capi.load_library()


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


@pytest.mark.parametrize("I,H,N", [(19, 32, 1), (3, 32, 33), (48, 64, 37), (235, 256, 64), (256, 256, 96),
                                   (1, 32, 32), (17, 160, 65), (40, 224, 33), (30, 128, 64)])
def test_one_step_matches_float64(I, H, N):
    """Both roles in one launch (the critic with another num_in), each role alone, and reset null / zero / set / mixed.  The last four
    shapes: one input; 5, 7 and 4 waves; N a multiple of 32; k-step counts with remainder 1 (17 and 89 k-steps) and 3 (79, 83)."""
    DeviceLstm, lstm_step, lib = _cells()
    Ic = I + 7 if I + 7 <= 256 else I - 7
    rnn_a, rnn_c = _rnn(I, H, 1), _rnn(Ic, H, 2)
    la, lc = DeviceLstm(rnn_a, DEV), DeviceLstm(rnn_c, DEV)
    gen = torch.Generator().manual_seed(I * 1000 + N)
    xa, xc = _uniform(gen, N, I), _uniform(gen, N, Ic)
    ha, ca, hc, cc = (torch.rand(N, H, generator=gen).to(DEV) * 2 - 1 for _ in range(4))
    mixed = (torch.arange(N) % 3 == 0).to(torch.uint8).to(DEV)
    pa, pc = lstm_params64(rnn_a), lstm_params64(rnn_c)
    for name, reset in (("null", None), ("zero", torch.zeros(N, dtype=torch.uint8, device=DEV)), ("set", torch.ones(N, dtype=torch.uint8, device=DEV)), ("mixed", mixed)):
        r = None if reset is None else reset.cpu().numpy()
        want_a = lstm_step64(pa, xa.cpu().numpy(), ha.cpu().numpy(), ca.cpu().numpy(), r)
        want_c = lstm_step64(pc, xc.cpu().numpy(), hc.cpu().numpy(), cc.cpu().numpy(), r)
        for roles in ("both", "actor", "critic"):
            full, outs = zip(*[_padded(N, H) for _ in range(4)])
            lstm_step(lib, la if roles != "critic" else None, lc if roles != "actor" else None, xa, xc, reset, (ha, ca), (outs[0], outs[1]), (hc, cc),
                      (outs[2], outs[3]), N, _stream())
            torch.cuda.synchronize()
            got = [o.cpu().double().numpy() for o in outs]
            if roles != "critic":
                err = max(np.abs(got[0] - want_a[0]).max(), np.abs(got[1] - want_a[1]).max())
                print(f"({I},{H},{N}) reset {name} {roles}: actor err {err:.3e}")
                assert err < TOL, (name, roles, err)
            else:
                assert np.isnan(got[0]).all() and np.isnan(got[1]).all()          # an absent role writes nothing
            if roles != "actor":
                err = max(np.abs(got[2] - want_c[0]).max(), np.abs(got[3] - want_c[1]).max())
                print(f"({I},{H},{N}) reset {name} {roles}: critic err {err:.3e}")
                assert err < TOL, (name, roles, err)
            else:
                assert np.isnan(got[2]).all() and np.isnan(got[3]).all()
            for f in full:
                assert torch.isnan(f[N:]).all()                                    # the sentinels behind row N are intact


@pytest.mark.parametrize("Ha,Hc", [(32, 96), (96, 32)])
def test_roles_of_different_hidden_size_in_one_launch(Ha, Hc):
    """The launch is sized for the wider memory: the narrower role's workgroups carry surplus waves, which stage and store nothing."""
    DeviceLstm, lstm_step, lib = _cells()
    I, Ic, N = 19, 26, 37
    rnn_a, rnn_c = _rnn(I, Ha, 1), _rnn(Ic, Hc, 2)
    la, lc = DeviceLstm(rnn_a, DEV), DeviceLstm(rnn_c, DEV)
    gen = torch.Generator().manual_seed(Ha)
    xa, xc = _uniform(gen, N, I), _uniform(gen, N, Ic)
    ha, ca = (torch.rand(N, Ha, generator=gen).to(DEV) * 2 - 1 for _ in range(2))
    hc, cc = (torch.rand(N, Hc, generator=gen).to(DEV) * 2 - 1 for _ in range(2))
    reset = (torch.arange(N) % 3 == 0).to(torch.uint8).to(DEV)
    r = reset.cpu().numpy()
    want = (lstm_step64(lstm_params64(rnn_a), xa.cpu().numpy(), ha.cpu().numpy(), ca.cpu().numpy(), r)
            + lstm_step64(lstm_params64(rnn_c), xc.cpu().numpy(), hc.cpu().numpy(), cc.cpu().numpy(), r))
    full, outs = zip(*[_padded(N, H) for H in (Ha, Ha, Hc, Hc)])
    lstm_step(lib, la, lc, xa, xc, reset, (ha, ca), (outs[0], outs[1]), (hc, cc), (outs[2], outs[3]), N, _stream())
    torch.cuda.synchronize()
    for i, (o, w) in enumerate(zip(outs, want)):
        err = np.abs(o.cpu().double().numpy() - w).max()
        print(f"hidden ({Ha},{Hc}) output {i}: err {err:.3e}")
        assert err < TOL, (i, err)
    for f in full:
        assert torch.isnan(f[N:]).all()


@pytest.mark.parametrize("I,H", [(70, 96)])
def test_exact_placement_of_every_weight_column(I, H):
    """"A = I with asymmetric B": with zero biases and a zero state, a one-hot ``x`` at column k makes the pre-activations exactly column
    k of ``W_ih``, so the outputs follow from that column alone (a lane-map or gate-order slip is O(0.1)); the same with ``x = 0`` and a
    one-hot ``h`` against ``W_hh``.  Row n of the batch carries the n-th tested column, so rows and columns cannot swap unseen."""
    DeviceLstm, lstm_step, lib = _cells()
    rnn = _rnn(I, H, 3)
    with torch.no_grad():
        rnn.bias_ih_l0.zero_(); rnn.bias_hh_l0.zero_()
        rnn.weight_ih_l0.uniform_(-2.0, 2.0); rnn.weight_hh_l0.uniform_(-2.0, 2.0)
    cell = DeviceLstm(rnn, DEV)

    def columns(width):
        ks = {0, width - 1}
        for m in range(32, width, 32):
            ks |= {m - 1, m}
        return sorted(k for k in ks if 0 <= k < width)

    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    for which, width, W in (("x", I, rnn.weight_ih_l0), ("h", H, rnn.weight_hh_l0)):
        ks = columns(width)
        N = len(ks)
        x, h = torch.zeros(N, I, device=DEV), torch.zeros(N, H, device=DEV)
        for n, k in enumerate(ks):
            (x if which == "x" else h)[n, k] = 1.0
        c = torch.zeros(N, H, device=DEV)
        h_out, c_out = torch.empty(N, H, device=DEV), torch.empty(N, H, device=DEV)
        lstm_step(lib, cell, None, x, None, None, (h, c), (h_out, c_out), None, None, N, _stream())
        torch.cuda.synchronize()
        W64 = W.detach().cpu().double().numpy()
        for n, k in enumerate(ks):
            col = W64[:, k].reshape(4, H)
            c_want = sig(col[0]) * np.tanh(col[2])
            h_want = sig(col[3]) * np.tanh(c_want)
            assert np.abs(c_out[n].cpu().double().numpy() - c_want).max() < TOL, (which, k)
            assert np.abs(h_out[n].cpu().double().numpy() - h_want).max() < TOL, (which, k)


def _run_24(cell, lstm_step, lib, xs, resets, N, H, graphed):
    """24 steps on ping-ponged state buffers from a zero state; returns the [24, N, H] outputs."""
    T = xs.shape[0]
    st = [(torch.zeros(N, H, device=DEV), torch.zeros(N, H, device=DEV)) for _ in range(2)]
    hs = torch.empty(T, N, H, device=DEV)
    x_in, r_in = torch.empty_like(xs[:2]), torch.empty_like(resets[:2])

    def two(t0, src_x, src_r, out):
        for j in range(2):
            lstm_step(lib, cell, None, src_x[j], None, src_r[j], st[j], st[1 - j], None, None, N, _stream())
            out[j].copy_(st[1 - j][0])

    if not graphed:
        for t in range(0, T, 2):
            two(t, xs[t:t + 2], resets[t:t + 2], hs[t:t + 2])
    else:
        out2 = torch.empty(2, N, H, device=DEV)
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            x_in.copy_(xs[:2]); r_in.copy_(resets[:2])
            with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                two(0, x_in, r_in, out2)
        torch.cuda.current_stream().wait_stream(side)
        for t in range(0, T, 2):
            x_in.copy_(xs[t:t + 2]); r_in.copy_(resets[t:t + 2])
            g.replay()
            hs[t:t + 2].copy_(out2)
    torch.cuda.synchronize()
    return hs, st[0][1].clone()


def test_24_steps_with_resets_match_float64_and_replay_bit_identically():
    I, H, N, T = 19, 64, 70, 24
    DeviceLstm, lstm_step, lib = _cells()
    rnn = _rnn(I, H, 4)
    cell = DeviceLstm(rnn, DEV)
    gen = torch.Generator().manual_seed(11)
    xs = _uniform(gen, T, N, I)
    resets = (torch.rand(T, N, generator=gen) < 0.1).to(torch.uint8).to(DEV)
    p = lstm_params64(rnn)
    h, c = np.zeros((N, H)), np.zeros((N, H))
    want = []
    for t in range(T):
        h, c = lstm_step64(p, xs[t].cpu().numpy(), h, c, resets[t].cpu().numpy())
        want.append(h)
    a, ca = _run_24(cell, lstm_step, lib, xs, resets, N, H, False)
    err = np.abs(a.cpu().double().numpy() - np.stack(want)).max()
    print(f"24 steps: err {err:.3e}")
    assert err < TOL
    assert np.abs(ca.cpu().double().numpy() - c).max() < TOL
    b, cb = _run_24(cell, lstm_step, lib, xs, resets, N, H, False)
    assert torch.equal(a, b) and torch.equal(ca, cb)
    g, cg = _run_24(cell, lstm_step, lib, xs, resets, N, H, True)
    assert torch.equal(a, g) and torch.equal(ca, cg)


def test_load_device_equals_create():
    I, H, N = 48, 64, 37
    DeviceLstm, lstm_step, lib = _cells()
    rnn = _rnn(I, H, 5)
    first = DeviceLstm(rnn, DEV)
    with torch.no_grad():
        for prm in rnn.parameters():
            prm.add_(0.05 * torch.randn_like(prm))
    fresh = DeviceLstm(rnn, DEV)                   # lg_lstm_create from the host copies of the new weights
    first.load_device()                            # lg_lstm_load_device from the CUDA parameters
    gen = torch.Generator().manual_seed(3)
    x, h, c = _uniform(gen, N, I), torch.rand(N, H, generator=gen).to(DEV), torch.rand(N, H, generator=gen).to(DEV)
    outs = []
    for cell in (first, fresh):
        ho, co = torch.empty(N, H, device=DEV), torch.empty(N, H, device=DEV)
        lstm_step(lib, cell, None, x, None, None, (h, c), (ho, co), None, None, N, _stream())
        outs.append((ho, co))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert np.abs(outs[0][0].cpu().double().numpy() - lstm_step64(lstm_params64(rnn), x.cpu().numpy(), h.cpu().numpy(), c.cpu().numpy())[0]).max() < TOL


# ---------------------------------------------------------------------------------------------------------------- edges of the cell
def test_saturated_gates_stay_finite_and_exact():
    """Pre-activations of 30, 100 and 1e4 of either sign in every gate (``saturating_bias``): the 1-ulp ``v_exp_f32`` overflows to inf or
    underflows to 0 there, and sigma / tanh must come out as exactly 0 / 1 / -1, never NaN.  24 steps from a zero state, eager.  c grows to
    about 15 in the units whose forget gate is pinned open, so the bar is TOL of the output scale, separately for h and c."""
    I, H, N, T = 19, 64, 37, 24
    DeviceLstm, lstm_step, lib = _cells()
    rnn = _rnn(I, H, 6)
    with torch.no_grad():
        rnn.bias_ih_l0.add_(torch.from_numpy(saturating_bias(H)).float().to(DEV))
    cell = DeviceLstm(rnn, DEV)
    gen = torch.Generator().manual_seed(13)
    xs = _uniform(gen, T, N, I)
    p = lstm_params64(rnn)
    st = [(torch.zeros(N, H, device=DEV), torch.zeros(N, H, device=DEV)) for _ in range(2)]
    h, c = np.zeros((N, H)), np.zeros((N, H))
    err_h = err_c = scale_h = scale_c = 0.0
    for t in range(T):
        lstm_step(lib, cell, None, xs[t], None, None, st[t & 1], st[1 - (t & 1)], None, None, N, _stream())
        torch.cuda.synchronize()
        got_h, got_c = st[1 - (t & 1)]
        h, c = lstm_step64(p, xs[t].cpu().numpy(), h, c)
        assert bool(torch.isfinite(got_h).all()) and bool(torch.isfinite(got_c).all()), t
        assert bool((got_h[:, 4::8] == 0.0).all()), t            # output gate at -1e4: sigma is exactly 0
        assert bool((got_c[:, 2::8] == 1.0).all()), t            # i at +1e4, f at -1e4 and g at +30 (tanh of 14.6 or more is 1.0f): c = 0 c + 1 * 1
        err_h, err_c = max(err_h, np.abs(got_h.cpu().double().numpy() - h).max()), max(err_c, np.abs(got_c.cpu().double().numpy() - c).max())
        scale_h, scale_c = max(scale_h, np.abs(h).max()), max(scale_c, np.abs(c).max())
    print(f"[observed] saturated gates: h err {err_h:.3e} (max |h| {scale_h:.3f}), c err {err_c:.3e} (max |c| {scale_c:.3f})")
    assert scale_c > 10.0                                        # the pinned-open forget gates did accumulate
    assert err_h < TOL * max(1.0, scale_h) and err_c < TOL * max(1.0, scale_c), (err_h, err_c)


@pytest.mark.parametrize("roles", ["both", "critic"])
def test_a_reset_row_ignores_its_stale_state(roles):
    """A row whose reset flag is set (any non-zero byte: 1, 2, 255) starts from zeros by SELECTION: NaN and Inf in its ``h_in`` / ``c_in``
    must not reach any output (0 * NaN is NaN: a multiply-by-mask would leak), nor NaN rows behind row N of ``x``, ``h_in``, ``c_in``.  The
    outputs are finite and bit-equal to the run with zeros in those places."""
    DeviceLstm, lstm_step, lib = _cells()
    I, Ic, H, N, extra = 19, 26, 64, 37, 5
    rnn_a, rnn_c = _rnn(I, H, 1), _rnn(Ic, H, 2)
    la, lc = (DeviceLstm(rnn_a, DEV) if roles == "both" else None), DeviceLstm(rnn_c, DEV)
    gen = torch.Generator().manual_seed(21)
    rows = torch.arange(N)
    flagged = rows % 3 == 0
    flags = torch.where(flagged, torch.tensor([1, 2, 255], dtype=torch.uint8)[(rows // 3) % 3], torch.zeros((), dtype=torch.uint8)).to(DEV)
    assert set(flags[flagged.to(DEV)].tolist()) == {1, 2, 255} and int(flags[~flagged.to(DEV)].max()) == 0

    def padded(width, poison, scale=1.0):
        """[N, width] uniform values as a view of a buffer whose rows behind N are NaN; ``poison``: NaN (and an Inf of either sign) in the
        reset rows.  Returns that view and one with zeros in the reset rows."""
        full = torch.full((N + extra, width), float("nan"))
        full[:N] = (torch.rand(N, width, generator=gen) * 2.0 - 1.0) * scale
        clean = full.clone()
        clean[:N][flagged] = 0.0
        if poison:
            full[:N][flagged] = float("nan")
            full[3, 1], full[6, width - 1] = float("inf"), float("-inf")
        return full.to(DEV)[:N], clean.to(DEV)[:N]

    xa, xc = padded(I, False, 3.0)[0], padded(Ic, False, 3.0)[0]
    states = [padded(H, True) for _ in range(4)]                 # h_a, c_a, h_c, c_c: (poisoned, zeros in the same places)
    results = []
    for k in (0, 1):
        ha, ca, hc, cc = (s[k] for s in states)
        full, outs = zip(*[_padded(N, H) for _ in range(4)])
        lstm_step(lib, la, lc, xa, xc, flags, (ha, ca), (outs[0], outs[1]), (hc, cc), (outs[2], outs[3]), N, _stream())
        torch.cuda.synchronize()
        for f in full:
            assert torch.isnan(f[N:]).all()
        results.append([o.clone() for o in (outs if roles == "both" else outs[2:])])
    for got, want in zip(*results):
        assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
    live = (~flagged).to(DEV)
    assert not torch.equal(results[0][-1][live], torch.zeros_like(results[0][-1][live]))
    want_c = lstm_step64(lstm_params64(rnn_c), xc.cpu().numpy(), states[2][1].cpu().numpy(), states[3][1].cpu().numpy(), flagged.numpy())
    assert np.abs(results[0][-2].cpu().double().numpy() - want_c[0]).max() < TOL and np.abs(results[0][-1].cpu().double().numpy() - want_c[1]).max() < TOL


# ---------------------------------------------------------------------------------------------------------------- RecurrentFusedActor
def _recurrent_policy(H=64, seed=7):
    from legged_games_gym_amd.rl import ActorCriticRecurrent
    torch.manual_seed(seed)
    ac = ActorCriticRecurrent(48, 48, 12, actor_hidden_dims=[128, 64, 32], critic_hidden_dims=[128, 64, 32], rnn_hidden_size=H).to(DEV)
    with torch.no_grad():
        ac.std.copy_(torch.linspace(0.3, 1.4, 12))
    return ac


def test_recurrent_fused_actor_follows_the_module_and_draws_the_fused_actors_noise():
    import copy
    from legged_games_gym_amd.rl import ActorCritic, FusedActor
    from legged_games_gym_amd.rl.recurrent_actor import RecurrentFusedActor
    N, T = 37, 6
    ac = _recurrent_policy()
    rfa = RecurrentFusedActor(ac, DEV, seed=5)
    gen = torch.Generator().manual_seed(9)
    obs = _uniform(gen, T, N, 48)
    dones = (torch.rand(T, N, generator=gen) < 0.25).to(DEV)
    dones[2] = dones[3]                                      # (an env done twice in a row is in there)
    # a policy with a zero output layer has mean 0, so its actions ARE std * eps: the draws of lg_policy_act and of the recurrent actor, bit for bit
    ac0 = copy.deepcopy(ac)
    plain_ac = ActorCritic(48, 48, 12, actor_hidden_dims=[128, 64, 32], critic_hidden_dims=[128, 64, 32]).to(DEV)
    with torch.no_grad():
        for m in (ac0.actor[6], plain_ac.actor[6]):
            m.weight.zero_(); m.bias.zero_()
        plain_ac.std.copy_(ac.std)
    rfa0, plain = RecurrentFusedActor(ac0, DEV, seed=5), FusedActor(plain_ac, DEV, seed=5)
    with torch.no_grad():
        for t in range(T):
            reset = dones[t - 1] if t else None
            actions, mean = (x.clone() for x in rfa.act_with_mean(obs[t], reset=reset))
            want = ac.act_inference(obs[t])
            ac.reset(dones[t])
            err = float((mean - want).abs().max())
            print(f"step {t}: mean err {err:.3e}")
            assert err < TOL, (t, err)
            noise = plain.act_with_mean(obs[t])[0].clone()
            noise0 = rfa0.act_with_mean(obs[t], reset=reset)[0].clone()
            assert torch.equal(noise, noise0), t
            assert float((actions - mean - noise).abs().max()) < 1e-6 and float(noise.abs().max()) > 0.1, t
    # an optimiser step, then sync_device(): the means follow the new weights
    opt = torch.optim.SGD(ac.parameters(), lr=0.05)
    ac.memory_a.hidden_states = None
    loss = ac.act_inference(obs[0]).square().sum() + ac.evaluate(obs[0]).sum()
    loss.backward()
    opt.step()
    rfa.sync_device()
    rfa.reset_states()
    ac.memory_a.hidden_states = None
    with torch.no_grad():
        for t in range(2):
            mean = rfa.act_with_mean(obs[t])[1].clone()
            want = ac.act_inference(obs[t])
            assert float((mean - want).abs().max()) < TOL, t
    # the critic memory: a step with critic observations advances it, a peek does not
    rfa.reset_states()
    ac.memory_c.hidden_states = None
    with torch.no_grad():
        _, _, h_c = rfa.act_with_mean(obs[0], obs[0])
        want = ac.memory_c(obs[0]).squeeze(0)
        assert float((h_c - want).abs().max()) < TOL
        before = [t.clone() for t in rfa.state_c[rfa._flip]]
        peek = rfa.peek_critic(obs[1]).clone()
        assert all(torch.equal(a, b) for a, b in zip(before, rfa.state_c[rfa._flip]))
        assert float((peek - ac.memory_c(obs[1]).squeeze(0)).abs().max()) < TOL


def test_default_policy_of_the_rough_task_through_the_wrapper():
    """``ActorCriticRecurrent``'s defaults on ``anymal_c_rough``: 235 observations, 256 units per memory, the 256-512-256-128-12 actor
    (dynamic LDS above 64 KB).  Four steps with dones (one env done twice in a row) against a float64 CPU copy of the module stepped with
    ``Memory.reset`` semantics: the means and the critic memory's output, TOL of the output scale."""
    import copy
    from legged_games_gym_amd.rl import ActorCriticRecurrent
    from legged_games_gym_amd.rl.recurrent_actor import RecurrentFusedActor
    N, T = 33, 4
    torch.manual_seed(8)
    ac = ActorCriticRecurrent(235, 235, 12, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128], rnn_hidden_size=256).to(DEV)
    assert ac.memory_a.rnn.hidden_size == 256 and ac.actor[0].in_features == 256
    ac64 = copy.deepcopy(ac).double().cpu()
    rfa = RecurrentFusedActor(ac, DEV, seed=5)
    gen = torch.Generator().manual_seed(10)
    obs = _uniform(gen, T, N, 235)
    dones = torch.rand(T, N, generator=gen) < 0.25
    dones[:, 32] = torch.tensor([False, True, True, False])      # the single row of the second workgroup: done twice in a row
    dones[0, 0] = True
    with torch.no_grad():
        for t in range(T):
            reset = dones[t - 1].to(DEV) if t else None
            _, mean, h_c = rfa.act_with_mean(obs[t], obs[t], reset)
            torch.cuda.synchronize()
            o64 = obs[t].cpu().double()
            want_mean = ac64.act_inference(o64).numpy()
            want_hc = ac64.memory_c(o64).squeeze(0).numpy()
            ac64.reset(dones[t])
            e_m, e_h = np.abs(mean.cpu().double().numpy() - want_mean).max(), np.abs(h_c.cpu().double().numpy() - want_hc).max()
            s_m, s_h = max(1.0, np.abs(want_mean).max()), max(1.0, np.abs(want_hc).max())
            print(f"[observed] rough default policy step {t}: mean err {e_m:.3e} (scale {s_m:.3f}), critic memory err {e_h:.3e} (scale {s_h:.3f})")
            assert e_m < TOL * s_m and e_h < TOL * s_h, (t, e_m, e_h)
        before = [x.clone() for pair in (rfa.state_a[rfa._flip], rfa.state_c[rfa._flip]) for x in pair]
        peek = rfa.peek_critic(obs[0], dones[T - 1].to(DEV)).clone()
        torch.cuda.synchronize()
        after = [x for pair in (rfa.state_a[rfa._flip], rfa.state_c[rfa._flip]) for x in pair]
        assert all(torch.equal(a, b) for a, b in zip(before, after))
        want_peek = ac64.memory_c(obs[0].cpu().double()).squeeze(0).numpy()      # (ac64 was reset with dones[T - 1] above)
        assert np.abs(peek.cpu().double().numpy() - want_peek).max() < TOL * max(1.0, np.abs(want_peek).max())


# ---------------------------------------------------------------------------------------------------------------- runner
def _runner(monkeypatch, hidden=64, graphed=True, **runner_keys):
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
    for name, value in runner_keys.items():                  # runner keys the constructor reads (fused_rollout)
        monkeypatch.setattr(train_cfg.runner, name, value, raising=False)
    env, _ = task_registry.make_env("anymal_c_flat", args)
    runner, _ = task_registry.make_alg_runner(env, "anymal_c_flat", args, log_root=None)
    runner.cfg["graphed_rollout"] = graphed
    # time-outs inside the first rollouts: every other env is a few steps from the end of its episode
    n = env.num_envs
    env.episode_length_buf[::2] = int(env.max_episode_length) - 2 - (torch.arange(0, n, 2, device=env.device) % 11)
    return env, runner


def _stats(runner):
    N, dev = runner.env.num_envs, runner.device
    sums = torch.zeros(3, device=dev)
    return {"cur_rew": torch.zeros(N, device=dev), "cur_len": torch.zeros(N, device=dev), "sum_rew": sums[0], "sum_len": sums[1], "count": sums[2], "_sums": sums}


def _check_storage_against_batch_mode(runner, tag):
    st, ac = runner.alg.storage, runner.alg.actor_critic
    assert int(st.dones.sum()) > 0, "no episode ended in the rollout: the reset path went untested"
    with torch.no_grad():
        (obs, cobs, act, val, adv, ret, lp, mu, sig, (hid_a, hid_c), masks), = list(st.recurrent_mini_batch_generator(1, 1))
        ac.act(obs, masks=masks, hidden_states=hid_a)
        new_mu = ac.action_mean
        new_val = ac.evaluate(cobs, masks=masks, hidden_states=hid_c)
    e_mu, e_val = float((new_mu - mu).abs().max()), float((new_val - val).abs().max())
    s_mu, s_val = max(1.0, float(new_mu.abs().max())), max(1.0, float(new_val.abs().max()))
    lp64 = (-(act.double() - mu.double()).square() / (2 * sig.double().square()) - sig.double().log() - 0.5 * np.log(2 * np.pi)).sum(-1, keepdim=True)
    e_lp = float((lp64 - lp.double()).abs().max())
    print(f"{tag}: mu err {e_mu:.3e} (scale {s_mu:.2f})  value err {e_val:.3e} (scale {s_val:.2f})  log-prob err {e_lp:.3e}  dones {int(st.dones.sum())}")
    assert e_mu < TOL * s_mu and e_val < TOL * s_val and e_lp < TOL, (tag, e_mu, e_val, e_lp)


def _snapshot(st):
    keep = [st.observations, st.actions, st.mu, st.sigma, st.actions_log_prob, st.values, st.rewards, st.dones] + list(st.initial_hidden_a) + list(st.initial_hidden_c)
    return [t.clone() for t in keep]


def test_runner_device_rollout_eager_and_graphed(monkeypatch, capsys):
    from legged_games_gym_amd.rl.recurrent_actor import RecurrentFusedActor
    env_g, run_g = _runner(monkeypatch, graphed=True)
    assert isinstance(run_g._fused, RecurrentFusedActor) and run_g._recurrent_rollout
    built = run_g._try_build_graphed_rollout()               # one eager warm-up rollout, then the capture
    assert built is not None, capsys.readouterr().out
    graph = built[0]
    graph.replay()
    run_g.alg.storage.step = run_g.num_steps_per_env
    torch.cuda.synchronize()
    assert float(run_g.alg.storage.initial_hidden_a[0].abs().max()) > 0.0      # the second rollout: a carried-in state
    _check_storage_against_batch_mode(run_g, "graphed")
    snap_g = _snapshot(run_g.alg.storage)
    hid_g = [t.clone() for pair in run_g.alg.actor_critic.get_hidden_states() for t in pair]

    env_e, run_e = _runner(monkeypatch, graphed=False)
    stats = _stats(run_e)
    with torch.inference_mode():
        run_e._rollout_steps(stats)                          # what the warm-up of the graphed runner did
        _check_storage_against_batch_mode(run_e, "eager, first rollout")
        run_e.alg.storage.clear()
        run_e._rollout_steps(stats)
    torch.cuda.synchronize()
    _check_storage_against_batch_mode(run_e, "eager, second rollout")
    snap_e = _snapshot(run_e.alg.storage)
    for i, (a, b) in enumerate(zip(snap_g, snap_e)):
        assert torch.equal(a, b), f"storage tensor {i} differs between the graph replay and the eager rollout"
    for a, b in zip(hid_g, [t for pair in run_e.alg.actor_critic.get_hidden_states() for t in pair]):
        assert torch.equal(a, b)                             # the torch memories were refreshed from the same device state

    for runner in (run_g, run_e):                            # two iterations each: graph replay and eager device rollout, torch BPTT update
        runner.alg.storage.clear()
        before = runner.alg.actor_critic.memory_a.rnn.weight_hh_l0.clone(), runner.alg.actor_critic.memory_c.rnn.weight_ih_l0.clone()
        losses, update = [], runner.alg.update
        monkeypatch.setattr(runner.alg, "update", lambda: losses.append(update()) or losses[-1])
        runner.learn(2)
        print("losses (value, surrogate):", losses)
        assert len(losses) == 2 and all(np.isfinite(v) for pair in losses for v in pair), losses
        ac = runner.alg.actor_critic
        assert all(bool(torch.isfinite(p).all()) for p in ac.parameters())
        assert not torch.equal(before[0], ac.memory_a.rnn.weight_hh_l0) and not torch.equal(before[1], ac.memory_c.rnn.weight_ih_l0)
    assert "unavailable" not in capsys.readouterr().out


def test_runner_falls_back_for_a_memory_the_cell_does_not_cover(monkeypatch, capsys):
    env, runner = _runner(monkeypatch, hidden=512)
    out = capsys.readouterr().out
    assert runner._fused is None and "device LSTM cell unavailable" in out and "512" in out
    before = runner.alg.actor_critic.memory_a.rnn.weight_hh_l0.clone()
    runner.learn(1)
    assert not torch.equal(before, runner.alg.actor_critic.memory_a.rnn.weight_hh_l0)


def test_generic_loop_carries_the_torch_memories_from_rollout_to_rollout(monkeypatch):
    """A recurrent policy without the device cell (``fused_rollout = False``) with ``graphed_rollout`` on and off: two consecutive
    rollouts from the same start leave the same storage and the same carried state, bit for bit.  (``Memory.forward`` leaves its state in
    a new tensor every step; a captured generic loop would start every replay from the state of its warm-up.)"""
    results = []
    for graphed in (True, False):
        env, runner = _runner(monkeypatch, graphed=graphed, fused_rollout=False)
        assert runner._fused is None and runner.alg.actor_critic.is_recurrent
        monkeypatch.setattr(runner.alg, "update", lambda r=runner: r.alg.storage.clear() or (0.0, 0.0))     # rollouts only
        torch.manual_seed(123)
        runner.learn(2)
        torch.cuda.synchronize()
        st = runner.alg.storage
        assert int(st.dones.sum()) > 0 and float(st.initial_hidden_a[0].abs().max()) > 0.0
        results.append(_snapshot(st) + [t.clone() for pair in runner.alg.actor_critic.get_hidden_states() for t in pair])
    for i, (a, b) in enumerate(zip(*results)):
        assert torch.equal(a, b), f"tensor {i} differs between graphed_rollout on and off"
