"""The GRU cell on the GPU (``lg_gru_*``, include/legged_recurrent_gru.h: k_gru_cell, k_gru_pack) against the float64 restatement of
``tests/gru_ref.py``, its exact gates, the stale state of reset rows, the placement of every weight block, capture and ``load_device``,
and ``RecurrentFusedActor(gru=True)`` through both runners and the game tasks with the key ``device_gru``.

The bar is ``TOL = 2e-5`` of the output scale, the one of ``tests/test_gpu_recurrent.py``.  The float32 ``nn.GRU`` stays within 2.2e-6 of
float64 on a CPU over these shapes with 33 rows, default weights and weights x 3 (0.11 of the bar); a cell that sums ``b_hn`` into the
bias of n is more than 1000 bars away (tests/test_gru_check.py)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests.gru_ref import gru_params64, gru_step64
from tests.noise_check import check_noise

pytestmark = pytest.mark.gpu
TOL = 2e-5
DEV = "cuda:0"
EXTRA = 5                    # NaN guard rows behind row N of every input and output


def _rnn(I, H, seed, gain=1.0):
    torch.manual_seed(seed)
    rnn = nn.GRU(I, H).to(DEV)
    if gain != 1.0:
        with torch.no_grad():
            rnn.weight_ih_l0.mul_(gain); rnn.weight_hh_l0.mul_(gain)
    return rnn


def _guarded(values):
    """``values`` [N, W] on the device as a view of a buffer whose rows behind N are NaN."""
    n, w = values.shape
    full = torch.full((n + EXTRA, w), float("nan"), device=DEV)
    full[:n] = values.to(DEV)
    return full[:n]


def _uniform(gen, n, w, scale=3.0):
    return _guarded((torch.rand(n, w, generator=gen) * 2.0 - 1.0) * scale)


def _padded(n, H):
    """An output buffer of ``n`` rows with NaN sentinels behind it."""
    t = torch.full((n + EXTRA, H), float("nan"), device=DEV)
    return t, t[:n]


def _cells():
    from legged_games_gym_amd import capi
    from legged_games_gym_amd.rl.recurrent_actor import DeviceGru, gru_step
    return (lambda rnn: DeviceGru(rnn, DEV)), gru_step, capi.load_gru_library()


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _np64(t):
    return t.detach().cpu().double().numpy()


def _one(gru_step, lib, cell, x, h, reset=None, role="actor"):
    """One launch of one role into a fresh guarded output; returns ``h_out``."""
    n, H = h.shape
    full, ho = _padded(n, H)
    if role == "actor":
        gru_step(lib, cell, None, x, None, reset, h, ho, None, None, n, _stream())
    else:
        gru_step(lib, None, cell, None, x, reset, None, None, h, ho, n, _stream())
    torch.cuda.synchronize()
    assert torch.isnan(full[n:]).all()
    return ho


# ---------------------------------------------------------------------------------------------------------------- the cell against float64
# every input count (1; 3 and 235: odd, the x / h boundary inside one k-step; 48; 256), every wave count (1, 2, 3, 5, 7, 8), odd and even
# K, the largest LDS block (256 + 256) and every N (one row; one short of, exactly and one past a block; three blocks) at least twice
CELL_CASES = [(1, 32, 1), (3, 64, 33), (48, 96, 31), (235, 256, 65), (256, 256, 32), (256, 224, 33), (3, 32, 65), (48, 160, 1), (235, 64, 32),
              (1, 96, 31), (48, 224, 65), (3, 160, 32)]


@pytest.mark.parametrize("I,H,N", CELL_CASES)
def test_one_step_matches_float64(I, H, N):
    """Both roles in one launch (the critic with another num_in), each role alone; reset null and mixed.  Inputs and outputs sit between NaN
    guard rows."""
    make, gru_step, lib = _cells()
    Ic = I + 7 if I + 7 <= 256 else I - 7
    rnn_a, rnn_c = _rnn(I, H, 1), _rnn(Ic, H, 2)
    la, lc = make(rnn_a), make(rnn_c)
    gen = torch.Generator().manual_seed(I * 1000 + N)
    xa, xc = _uniform(gen, N, I), _uniform(gen, N, Ic)
    ha, hc = _uniform(gen, N, H, 1.0), _uniform(gen, N, H, 1.0)
    mixed = (torch.arange(N) % 3 == 0).to(torch.uint8).to(DEV)
    pa, pc = gru_params64(rnn_a), gru_params64(rnn_c)
    worst = 0.0
    for name, reset in (("null", None), ("mixed", mixed)):
        r = None if reset is None else reset.cpu().numpy()
        want_a, want_c = gru_step64(pa, _np64(xa), _np64(ha), r), gru_step64(pc, _np64(xc), _np64(hc), r)
        for roles in ("both", "actor", "critic"):
            full, outs = zip(*[_padded(N, H) for _ in range(2)])
            gru_step(lib, la if roles != "critic" else None, lc if roles != "actor" else None, xa, xc, reset, ha, outs[0], hc, outs[1], N, _stream())
            torch.cuda.synchronize()
            got = [_np64(o) for o in outs]
            for present, mine, want, who in ((roles != "critic", got[0], want_a, "actor"), (roles != "actor", got[1], want_c, "critic")):
                if present:
                    err = np.abs(mine - want).max()
                    worst = max(worst, err)
                    assert np.isfinite(mine).all()
                    assert err < TOL, (name, roles, who, err)
                else:
                    assert np.isnan(mine).all()                                    # an absent role writes nothing
            for f in full:
                assert torch.isnan(f[N:]).all()                                    # the sentinels behind row N are intact
    print(f"[observed] GRU cell ({I},{H},{N}): worst err {worst:.3e} = {worst / TOL:.3f} of the bar")


def test_one_step_with_weights_times_three_matches_float64():
    make, gru_step, lib = _cells()
    for I, H, N in ((48, 256, 33), (235, 96, 33)):
        rnn = _rnn(I, H, 3, gain=3.0)
        cell = make(rnn)
        gen = torch.Generator().manual_seed(5)
        x, h = _uniform(gen, N, I), _uniform(gen, N, H, 1.0)
        reset = (torch.arange(N) % 4 == 1).to(torch.uint8).to(DEV)
        ho = _one(gru_step, lib, cell, x, h, reset)
        want = gru_step64(gru_params64(rnn), _np64(x), _np64(h), reset.cpu().numpy())
        err = np.abs(_np64(ho) - want).max()
        print(f"[observed] GRU cell weights x 3 ({I},{H},{N}): err {err:.3e} = {err / TOL:.3f} of the bar")
        assert err < TOL


@pytest.mark.parametrize("Ha,Hc", [(32, 256), (256, 64)])
def test_roles_of_different_hidden_size_in_one_launch(Ha, Hc):
    """The launch is sized for the wider role; the narrower one's surplus waves only meet the barrier.  Each role is bit-identical to that
    role alone, and within the bar of float64."""
    make, gru_step, lib = _cells()
    I, Ic, N = 19, 26, 37
    rnn_a, rnn_c = _rnn(I, Ha, 1), _rnn(Ic, Hc, 2)
    la, lc = make(rnn_a), make(rnn_c)
    gen = torch.Generator().manual_seed(Ha)
    xa, xc = _uniform(gen, N, I), _uniform(gen, N, Ic)
    ha, hc = _uniform(gen, N, Ha, 1.0), _uniform(gen, N, Hc, 1.0)
    reset = (torch.arange(N) % 3 == 0).to(torch.uint8).to(DEV)
    r = reset.cpu().numpy()
    (fa, oa), (fc, oc) = _padded(N, Ha), _padded(N, Hc)
    gru_step(lib, la, lc, xa, xc, reset, ha, oa, hc, oc, N, _stream())
    torch.cuda.synchronize()
    assert torch.isnan(fa[N:]).all() and torch.isnan(fc[N:]).all()
    alone_a, alone_c = _one(gru_step, lib, la, xa, ha, reset), _one(gru_step, lib, lc, xc, hc, reset, role="critic")
    assert bool(torch.isfinite(oa).all()) and torch.equal(oa, alone_a) and bool(torch.isfinite(oc).all()) and torch.equal(oc, alone_c)
    for o, want in ((oa, gru_step64(gru_params64(rnn_a), _np64(xa), _np64(ha), r)), (oc, gru_step64(gru_params64(rnn_c), _np64(xc), _np64(hc), r))):
        err = np.abs(_np64(o) - want).max()
        print(f"[observed] GRU hidden ({Ha},{Hc}): err {err:.3e}")
        assert err < TOL


# ---------------------------------------------------------------------------------------------------------------- exact gates
def _gate_bias(rnn, gate, value):
    """Add ``value`` to ``b_i<gate>`` (gate 0 = r, 1 = z, 2 = n) of every unit."""
    H = rnn.hidden_size
    with torch.no_grad():
        rnn.bias_ih_l0[gate * H:(gate + 1) * H] += value


def test_a_saturated_update_gate_returns_h_in_bit_for_bit():
    """``b_iz = +1e4``: z is exactly 1 and ``h' = (1 - z) n + z h`` returns ``h_in`` on live rows, exactly 0 on reset rows."""
    make, gru_step, lib = _cells()
    I, H, N = 19, 96, 37
    rnn = _rnn(I, H, 4)
    _gate_bias(rnn, 1, 1e4)
    gen = torch.Generator().manual_seed(2)
    x, h = _uniform(gen, N, I), _uniform(gen, N, H, 1.0)
    reset = (torch.arange(N) % 3 == 0).to(DEV)
    ho = _one(gru_step, lib, make(rnn), x, h, reset.to(torch.uint8))
    assert torch.equal(ho[~reset], h[~reset]) and float(h[~reset].abs().min()) > 0.0
    assert bool((ho[reset] == 0.0).all())
    assert torch.equal(_one(gru_step, lib, make(rnn), x, h), h)


def test_closed_gates_return_the_candidate_of_x_alone():
    """``b_iz = b_ir = -1e4``: z and r are exactly 0, so ``h' = n = tanh(W_in x + b_in)``: the same bits for two different ``h_in`` and for
    two different ``b_hn`` (r multiplies the whole h part of n, ``b_hn`` included), within the bar of float64."""
    make, gru_step, lib = _cells()
    I, H, N = 19, 96, 37
    rnn = _rnn(I, H, 4)
    _gate_bias(rnn, 0, -1e4); _gate_bias(rnn, 1, -1e4)
    cell = make(rnn)
    gen = torch.Generator().manual_seed(2)
    x, h1, h2 = _uniform(gen, N, I), _uniform(gen, N, H, 1.0), _uniform(gen, N, H, 1.0)
    a, b = _one(gru_step, lib, cell, x, h1), _one(gru_step, lib, cell, x, h2)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b) and not torch.equal(h1, h2)
    with torch.no_grad():
        rnn.bias_hh_l0[2 * H:] += torch.linspace(-2.0, 2.0, H, device=DEV)
    cell.load_device()
    c = _one(gru_step, lib, cell, x, h1)
    assert torch.equal(a, c)
    p = gru_params64(rnn)
    want = np.tanh(_np64(x) @ p[0][2 * H:].T + p[2][2 * H:])
    err = np.abs(_np64(a) - want).max()
    print(f"[observed] GRU closed gates: err {err:.3e} = {err / TOL:.3f} of the bar")
    assert err < TOL and float(np.abs(want).max()) > 0.5


def test_pre_activations_at_1e4_stay_finite():
    """Every pre-activation at +-1e4 (sign by unit and gate; the h part of n with the sign of its x part, so that the two do not cancel):
    sigma and tanh come out as exactly 0 / 1 / -1, never NaN, and the outputs are float64's."""
    make, gru_step, lib = _cells()
    I, H, N = 19, 96, 37
    rnn = _rnn(I, H, 4)
    with torch.no_grad():
        unit, gate = torch.arange(3 * H) % H, torch.arange(3 * H) // H
        sign = torch.where((unit >> gate) & 1 == 0, 1.0, -1.0).to(DEV)      # bit g of the unit: every combination of the three gates' signs
        rnn.bias_ih_l0.add_(1e4 * sign)
        rnn.bias_hh_l0[2 * H:] += 1e4 * sign[2 * H:]
    gen = torch.Generator().manual_seed(2)
    x, h = _uniform(gen, N, I), _uniform(gen, N, H, 1.0)
    reset = (torch.arange(N) % 3 == 0).to(torch.uint8).to(DEV)
    ho = _one(gru_step, lib, make(rnn), x, h, reset)
    want = gru_step64(gru_params64(rnn), _np64(x), _np64(h), reset.cpu().numpy())
    assert bool(torch.isfinite(ho).all()) and np.abs(_np64(ho) - want).max() < TOL
    assert {float(v) for v in ho[1].unique()} >= {1.0, -1.0}                    # a live row: z = 0 units return n = +-1 exactly


def test_a_reset_row_ignores_its_stale_state():
    """Flag bytes 1, 2 and 255 start a row from zeros by selection: NaN and +-Inf in its ``h_in`` reach no output, and the outputs are
    bit-equal to the run with zeros in those places (both roles); live rows are untouched."""
    make, gru_step, lib = _cells()
    I, Ic, H, N = 19, 26, 160, 37
    rnn_a, rnn_c = _rnn(I, H, 1), _rnn(Ic, H, 2)
    la, lc = make(rnn_a), make(rnn_c)
    gen = torch.Generator().manual_seed(21)
    rows = torch.arange(N)
    flagged = rows % 3 == 0
    flags = torch.where(flagged, torch.tensor([1, 2, 255], dtype=torch.uint8)[(rows // 3) % 3], torch.zeros((), dtype=torch.uint8)).to(DEV)
    assert set(flags[flagged.to(DEV)].tolist()) == {1, 2, 255}

    def state():
        values = torch.rand(N, H, generator=gen) * 2.0 - 1.0
        clean, poisoned = values.clone(), values.clone()
        clean[flagged] = 0.0
        poisoned[flagged] = float("nan")
        poisoned[3, 1], poisoned[6, H - 1], poisoned[9, 100] = float("inf"), float("-inf"), float("inf")
        return _guarded(poisoned), _guarded(clean)

    xa, xc = _uniform(gen, N, I), _uniform(gen, N, Ic)
    states = [state() for _ in range(2)]
    results = []
    for k in (0, 1):
        ha, hc = (s[k] for s in states)
        full, outs = zip(*[_padded(N, H) for _ in range(2)])
        gru_step(lib, la, lc, xa, xc, flags, ha, outs[0], hc, outs[1], N, _stream())
        torch.cuda.synchronize()
        for f in full:
            assert torch.isnan(f[N:]).all()
        results.append([o.clone() for o in outs])
    for got, want in zip(*results):
        assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
    for got, rnn, x, st in ((results[0][0], rnn_a, xa, states[0][1]), (results[0][1], rnn_c, xc, states[1][1])):
        assert np.abs(_np64(got) - gru_step64(gru_params64(rnn), _np64(x), _np64(st), flagged.numpy())).max() < TOL


@pytest.mark.parametrize("I,H", [(3, 32), (235, 64)])
def test_exact_placement_of_every_weight_column(I, H):
    """One-hot ``x`` (then one-hot ``h``) at column k with zero biases except a large ``b_hn``: with a zero state and one-hot ``x`` the
    outputs follow from column k of ``W_ir`` (through r on ``b_hn``), ``W_iz`` and ``W_in``; with one-hot ``h`` from column k of ``W_hr``,
    ``W_hz`` and ``W_hn``.  A block in the wrong gate or in the wrong half of n shows.  Row n of the batch carries the n-th tested column."""
    make, gru_step, lib = _cells()
    rnn = _rnn(I, H, 3)
    with torch.no_grad():
        rnn.bias_ih_l0.zero_(); rnn.bias_hh_l0.zero_()
        rnn.bias_hh_l0[2 * H:] = 0.75                                  # b_hn: makes r visible in n on the x side
        rnn.weight_ih_l0.uniform_(-2.0, 2.0); rnn.weight_hh_l0.uniform_(-2.0, 2.0)
    cell = make(rnn)

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
        h_out = _one(gru_step, lib, cell, x, h)
        W64 = _np64(W)
        for n, k in enumerate(ks):
            col = W64[:, k].reshape(3, H)
            r, z = sig(col[0]), sig(col[1])
            if which == "x":
                want = (1.0 - z) * np.tanh(col[2] + r * 0.75)
            else:
                want = (1.0 - z) * np.tanh(r * (col[2] + 0.75)) + z * _np64(h[n])
            assert np.abs(_np64(h_out[n]) - want).max() < TOL, (which, k)
    # the control of this test: the two halves of n swapped, or r and z swapped, are far from what is asserted
    col = _np64(rnn.weight_ih_l0)[:, 0].reshape(3, H)
    right = (1.0 - sig(col[1])) * np.tanh(col[2] + sig(col[0]) * 0.75)
    assert np.abs(right - (1.0 - sig(col[1])) * np.tanh(sig(col[0]) * (col[2] + 0.75))).max() > 1000 * TOL
    assert np.abs(right - (1.0 - sig(col[0])) * np.tanh(col[2] + sig(col[1]) * 0.75)).max() > 1000 * TOL


def test_load_device_equals_create_and_the_next_launch_sees_new_parameters():
    I, H, N = 48, 224, 37
    make, gru_step, lib = _cells()
    rnn = _rnn(I, H, 5)
    first = make(rnn)
    gen = torch.Generator().manual_seed(3)
    x, h = _uniform(gen, N, I), _uniform(gen, N, H, 1.0)
    before = _one(gru_step, lib, first, x, h)
    with torch.no_grad():
        for prm in rnn.parameters():
            prm.add_(0.05 * torch.randn_like(prm))
    stale = _one(gru_step, lib, first, x, h)                     # the handle owns its operands: the module moved, the handle did not
    assert torch.equal(stale, before)
    fresh = make(rnn)                                            # lg_gru_create from the host copies of the new weights
    first.load_device()                                          # lg_gru_load_device from the CUDA parameters
    a, b = _one(gru_step, lib, first, x, h), _one(gru_step, lib, fresh, x, h)
    assert torch.equal(a, b) and not torch.equal(a, before)
    assert np.abs(_np64(a) - gru_step64(gru_params64(rnn), _np64(x), _np64(h))).max() < TOL


def test_aliasing_is_refused_and_nothing_is_written():
    make, gru_step, lib = _cells()
    I, H, N = 19, 64, 33
    cell = make(_rnn(I, H, 1))
    x, h = torch.zeros(N, I, device=DEV), torch.zeros(N, H, device=DEV)
    rc = lib.lg_gru_step(cell.handle, None, x.data_ptr(), None, None, h.data_ptr(), h.data_ptr(), None, None, N, _stream())
    assert rc == -2 and b"alias" in lib.lg_gru_last_error()
    rc = lib.lg_gru_step(None, cell.handle, None, x.data_ptr(), None, None, None, h.data_ptr(), h.data_ptr(), N, _stream())
    assert rc == -2 and b"alias" in lib.lg_gru_last_error()
    torch.cuda.synchronize()
    assert float(h.abs().max()) == 0.0


def _run_24(cell, gru_step, lib, xs, resets, N, H, graphed):
    """24 steps on ping-ponged state buffers from a zero state; returns the [24, N, H] outputs."""
    T = xs.shape[0]
    st = [torch.zeros(N, H, device=DEV) for _ in range(2)]
    hs = torch.empty(T, N, H, device=DEV)
    x_in, r_in = torch.empty_like(xs[:2]), torch.empty_like(resets[:2])

    def two(src_x, src_r, out):
        for j in range(2):
            gru_step(lib, cell, None, src_x[j], None, src_r[j], st[j], st[1 - j], None, None, N, _stream())
            out[j].copy_(st[1 - j])

    if not graphed:
        for t in range(0, T, 2):
            two(xs[t:t + 2], resets[t:t + 2], hs[t:t + 2])
    else:
        out2 = torch.empty(2, N, H, device=DEV)
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            x_in.copy_(xs[:2]); r_in.copy_(resets[:2])
            with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                two(x_in, r_in, out2)
        torch.cuda.current_stream().wait_stream(side)
        for t in range(0, T, 2):
            x_in.copy_(xs[t:t + 2]); r_in.copy_(resets[t:t + 2])
            g.replay()
            hs[t:t + 2].copy_(out2)
    torch.cuda.synchronize()
    return hs


def test_24_steps_with_resets_match_float64_and_replay_bit_identically():
    I, H, N, T = 19, 96, 70, 24
    make, gru_step, lib = _cells()
    rnn = _rnn(I, H, 4)
    cell = make(rnn)
    gen = torch.Generator().manual_seed(11)
    xs = (torch.rand(T, N, I, generator=gen) * 6.0 - 3.0).to(DEV)
    resets = (torch.rand(T, N, generator=gen) < 0.1).to(torch.uint8).to(DEV)
    a = _run_24(cell, gru_step, lib, xs, resets, N, H, False)
    p, h, worst = gru_params64(rnn), np.zeros((N, H)), 0.0
    for t in range(T):
        h = gru_step64(p, _np64(xs[t]), h, resets[t].cpu().numpy())
        worst = max(worst, np.abs(_np64(a[t]) - h).max())
    print(f"[observed] GRU 24 steps: worst err {worst:.3e} = {worst / TOL:.3f} of the bar")
    assert worst < TOL and float(a[-1].abs().max()) > 0.0
    g = _run_24(cell, gru_step, lib, xs, resets, N, H, True)
    assert torch.equal(a, g)


# ---------------------------------------------------------------------------------------------------------------- RecurrentFusedActor(gru=True)
def _recurrent_policy(H=64, seed=7, num_obs=48, num_actions=12, hidden=(128, 64, 32)):
    from legged_games_gym_amd.rl import ActorCriticRecurrent
    torch.manual_seed(seed)
    ac = ActorCriticRecurrent(num_obs, num_obs, num_actions, actor_hidden_dims=list(hidden), critic_hidden_dims=list(hidden), rnn_type="gru",
                              rnn_hidden_size=H).to(DEV)
    with torch.no_grad():
        ac.std.copy_(torch.linspace(0.3, 1.4, num_actions))
    return ac


def test_recurrent_fused_actor_follows_the_module_and_draws_the_fused_actors_noise():
    from legged_games_gym_amd import capi
    from legged_games_gym_amd.rl.recurrent_actor import DeviceGru, RecurrentFusedActor
    N, T, seed = 37, 4, 5
    ac = _recurrent_policy()
    assert isinstance(ac.memory_a.rnn, nn.GRU) and isinstance(ac.memory_c.rnn, nn.GRU)
    ac64 = copy.deepcopy(ac).double().cpu()
    with pytest.raises(ValueError, match="no device LSTM cell for a GRU memory"):
        RecurrentFusedActor(ac, DEV, seed=seed)                  # without gru: today's refusal
    rfa = RecurrentFusedActor(ac, DEV, seed=seed, gru=True)
    assert rfa.gru is True and rfa.wide is False and rfa.recurrent is True and isinstance(rfa.lstm_a, DeviceGru) and isinstance(rfa.lstm_c, DeviceGru)
    assert rfa.cell_lib is capi.load_gru_library() and rfa.lib is capi.load_library() and rfa.fused.lib is capi.load_library() and not rfa.fused.wide
    gen = torch.Generator().manual_seed(9)
    obs = (torch.rand(T, N, 48, generator=gen) * 6.0 - 3.0).to(DEV)
    dones = torch.rand(T, N, generator=gen) < 0.25
    dones[:, 32] = torch.tensor([False, True, True, False])      # done twice in a row
    dones[0, 0] = True
    std, report = _np64(ac.std), {}
    with torch.no_grad():
        for t in range(T):
            reset = dones[t - 1].to(DEV) if t else None
            actions, mean, h_c = rfa.act_with_mean(obs[t], obs[t], reset)
            torch.cuda.synchronize()
            (h_a,), _ = rfa.hidden_states()
            o64 = obs[t].cpu().double()
            want_mean = ac64.act_inference(o64).numpy()
            want_ha = ac64.memory_a.hidden_states.squeeze(0).numpy().copy()      # (Memory.reset below zeroes rows of the state where it is)
            want_hc = ac64.memory_c(o64).squeeze(0).numpy()
            ac64.reset(dones[t])
            e_m, e_a, e_c = (np.abs(_np64(g) - w).max() for g, w in ((mean, want_mean), (h_a[0], want_ha), (h_c, want_hc)))
            s_m = max(1.0, np.abs(want_mean).max())
            print(f"[observed] GRU wrapper step {t}: mean err {e_m:.3e} (scale {s_m:.3f}), h_a err {e_a:.3e}, h_c err {e_c:.3e}")
            assert e_m < TOL * s_m and e_a < TOL and e_c < TOL, (t, e_m, e_a, e_c)
            check_noise(actions.cpu().numpy(), mean.cpu().numpy(), std, seed, t + 1, report)      # FusedActor's stream: host steps 1, 2, ..
        print("[observed] GRU wrapper noise: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(report.items())))
        # peek_critic leaves the carried state
        before = [x.clone() for st in (rfa.state_a[rfa._flip], rfa.state_c[rfa._flip]) for x in st]
        assert len(before) == 2                                  # one tensor per memory
        peek = rfa.peek_critic(obs[0], dones[T - 1].to(DEV)).clone()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(before, [x for st in (rfa.state_a[rfa._flip], rfa.state_c[rfa._flip]) for x in st]))
        want_peek = ac64.memory_c(obs[0].cpu().double()).squeeze(0).numpy()      # (ac64 was reset with dones[T - 1] above)
        assert np.abs(_np64(peek) - want_peek).max() < TOL
        # publish_states: the torch memories are tensors equal to the device state (rows of the next reset zeroed)
        rfa.publish_states()
        (ha,), (hc,) = rfa.hidden_states()
        assert torch.is_tensor(ac.memory_a.hidden_states) and torch.is_tensor(ac.memory_c.hidden_states)
        assert ha.shape == (1, N, 64) and torch.equal(ac.memory_a.hidden_states, ha) and torch.equal(ac.memory_c.hidden_states, hc)
        flags = dones[T - 1].to(DEV)
        rfa.publish_states(flags)
        assert bool((ac.memory_a.hidden_states[0, flags] == 0.0).all()) and torch.equal(ac.memory_a.hidden_states[0, ~flags], ha[0, ~flags])
        want = ac.act_inference(obs[0])                          # the torch module steps from the published state
        assert float((rfa.act_with_mean(obs[0], reset=flags)[1] - want).abs().max()) < TOL * max(1.0, float(want.abs().max()))
        # an actor-only step keeps both critic slots current; hold_slot reads from the same slot again
        flip = rfa._flip
        rfa.step_memories(obs[0])
        assert rfa._flip == 1 - flip and torch.equal(rfa.state_c[0][0], rfa.state_c[1][0])
        rfa.hold_slot()
        assert rfa._flip == flip and torch.equal(rfa.state_a[0][0], rfa.state_a[1][0])
        rfa.reset_critic_state()
        assert float(rfa.state_c[0][0].abs().max()) == 0.0 and float(rfa.state_a[rfa._flip][0].abs().max()) > 0.0
        rfa.reset_states()
        assert float(rfa.state_a[0][0].abs().max()) == 0.0 and float(rfa.state_a[1][0].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- OnPolicyRunner
def _runner(monkeypatch, hidden=64, graphed=True, **runner_keys):
    from legged_games_gym_amd.envs import task_registry
    from legged_games_gym_amd.utils import get_args
    from legged_games_gym_amd.utils.helpers import apply_policy_args
    _, train_cfg = task_registry.get_cfgs("anymal_c_flat")
    args = get_args(["--task", "anymal_c_flat", "--num_envs", "64", "--headless", "--sim_device", DEV, "--rl_device", DEV,
                     "--policy_class_name", "ActorCriticRecurrent", "--rnn_type", "gru", "--rnn_hidden_size", str(hidden)])
    for obj, name in ((train_cfg.runner, "policy_class_name"), (train_cfg.runner, "num_steps_per_env"), (train_cfg.runner, "max_iterations"),
                      (train_cfg.policy, "rnn_hidden_size"), (train_cfg.policy, "rnn_type")):      # the registered cfg is shared: put every field back afterwards
        monkeypatch.setattr(obj, name, getattr(obj, name, None), raising=False)
    train_cfg.runner.num_steps_per_env = 8
    apply_policy_args(train_cfg, args)
    for name, value in runner_keys.items():
        monkeypatch.setattr(train_cfg.runner, name, value, raising=False)
    env, _ = task_registry.make_env("anymal_c_flat", args)
    runner, _ = task_registry.make_alg_runner(env, "anymal_c_flat", args, log_root=None)
    runner.cfg["graphed_rollout"] = graphed
    n = env.num_envs                                         # time-outs inside the first rollouts
    env.episode_length_buf[::2] = int(env.max_episode_length) - 2 - (torch.arange(0, n, 2, device=env.device) % 11)
    return env, runner


def test_runner_device_rollout_with_gru_memories_eager_and_graphed(monkeypatch, capsys):
    from legged_games_gym_amd.rl.recurrent_actor import RecurrentFusedActor
    from tests.test_gpu_recurrent import _check_storage_against_batch_mode, _snapshot, _stats
    env_g, run_g = _runner(monkeypatch, graphed=True, device_gru=True)
    assert isinstance(run_g._fused, RecurrentFusedActor) and run_g._fused.gru and run_g._recurrent_rollout
    assert isinstance(run_g.alg.actor_critic.memory_a.rnn, nn.GRU) and run_g.alg.actor_critic.memory_a.rnn.hidden_size == 64
    built = run_g._try_build_graphed_rollout()               # one eager warm-up rollout, then the capture
    assert built is not None, capsys.readouterr().out
    built[0].replay()
    run_g.alg.storage.step = run_g.num_steps_per_env
    torch.cuda.synchronize()
    assert len(run_g.alg.storage.initial_hidden_a) == 1 and float(run_g.alg.storage.initial_hidden_a[0].abs().max()) > 0.0      # a carried-in state
    _check_storage_against_batch_mode(run_g, "GRU, graphed")
    snap_g = _snapshot(run_g.alg.storage)
    hid_g = [t.clone() for t in run_g.alg.actor_critic.get_hidden_states()]
    assert all(torch.is_tensor(t) for t in hid_g)

    env_e, run_e = _runner(monkeypatch, graphed=False, device_gru=True)
    stats = _stats(run_e)
    with torch.inference_mode():
        run_e._rollout_steps(stats)                          # what the warm-up of the graphed runner did
        _check_storage_against_batch_mode(run_e, "GRU, eager, first rollout")
        run_e.alg.storage.clear()
        run_e._rollout_steps(stats)
    torch.cuda.synchronize()
    _check_storage_against_batch_mode(run_e, "GRU, eager, second rollout")
    for i, (a, b) in enumerate(zip(snap_g, _snapshot(run_e.alg.storage))):
        assert torch.equal(a, b), f"storage tensor {i} differs between the graph replay and the eager rollout"
    for a, b in zip(hid_g, run_e.alg.actor_critic.get_hidden_states()):
        assert torch.equal(a, b)                             # the torch memories were refreshed from the same device state

    run_g.alg.storage.clear()                                # two iterations: graph replay, torch BPTT update
    ac = run_g.alg.actor_critic
    before = ac.memory_a.rnn.weight_hh_l0.clone(), ac.memory_c.rnn.weight_ih_l0.clone()
    losses, update = [], run_g.alg.update
    monkeypatch.setattr(run_g.alg, "update", lambda: losses.append(update()) or losses[-1])
    run_g.learn(2)
    assert len(losses) == 2 and all(np.isfinite(v) for pair in losses for v in pair), losses
    assert all(bool(torch.isfinite(p).all()) for p in ac.parameters())
    assert not torch.equal(before[0], ac.memory_a.rnn.weight_hh_l0) and not torch.equal(before[1], ac.memory_c.rnn.weight_ih_l0)
    assert "unavailable" not in capsys.readouterr().out


def test_runner_without_the_key_says_what_it_says_today_and_learns(monkeypatch, capsys):
    env, runner = _runner(monkeypatch)
    out = capsys.readouterr().out
    line, = [l for l in out.splitlines() if "unavailable" in l]
    assert runner._fused is None and line.startswith("[runner] device LSTM cell unavailable (GRU memory (the device cell is an LSTM)); torch policy in the rollout")
    before = runner.alg.actor_critic.memory_a.rnn.weight_hh_l0.clone()
    runner.learn(1)
    assert not torch.equal(before, runner.alg.actor_critic.memory_a.rnn.weight_hh_l0)


# ---------------------------------------------------------------------------------------------------------------- high_level_game
N_GAME = 33


def _game_policy(units=64, hidden=(64, 64, 32), seed=6):
    ac = _recurrent_policy(units, seed, num_obs=19, num_actions=6, hidden=hidden)
    with torch.no_grad():
        ac.std.copy_(torch.tensor((0.6, 0.6, 1.0, 1.0, 1.0, 1.0)))
        ac.actor[-1].bias.copy_(torch.tensor((0.7, -0.7, 2.2, 0.0, 1.5, -1.5)))
    return ac


def test_game_step_policy_equals_its_pieces_and_the_graphed_step_the_eager_one(tmp_path, capsys):
    """``high_level_game`` with a GRU policy.  A: ``step_policy(RecurrentFusedActor(gru=True))`` (``lg_gru_step`` -> ``lg_game_lstm_act`` ->
    ``lg_step`` -> post).  B, identically seeded: ``lg_gru_step`` -> ``lg_lstm_actor_act`` -> ``env.step(command)`` (``lg_game_pre`` +
    ``lg_policy_act`` inside).  Two steps with a reset forced in between; then four replays of the graphed policy step on A against four
    eager ``step_policy`` on B."""
    from legged_games_gym_amd.rl.recurrent_actor import RecurrentFusedActor
    from tests.test_gpu_game import make_game, write_ll_checkpoint
    from tests.test_gpu_game_recurrent import _assert_same_state, _same_memories, _two_envs
    n = N_GAME
    A, B = _two_envs(tmp_path, make_game, n=n)
    ac = _game_policy()
    fa, fb = (RecurrentFusedActor(ac, DEV, seed=21, num_envs=n, gru=True) for _ in range(2))
    assert fa.gru and A.shared_actor_launch(fa) is True          # the main-library actor handle: lg_game_lstm_act serves a GRU memory's h
    forced = torch.arange(3, n, 5, device=DEV)
    sample = torch.empty(n, 6, device=DEV)
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
        if k == 1:                                                                 # a reset row's memory started from zero
            fresh = RecurrentFusedActor(ac, DEV, seed=21, num_envs=n, gru=True)
            fresh.step_memories(obs_b, obs_b)
            rows = flags.nonzero().flatten()
            assert set(forced.tolist()) <= set(rows.tolist()) and len(rows) < n
            for mine, zero in zip(fa.hidden_states(), fresh.hidden_states()):
                assert len(mine) == 1 and torch.equal(mine[0][0, rows], zero[0][0, rows])
            live = (~flags).nonzero().flatten()
            assert not torch.equal(fa.hidden_states()[0][0][0, live], fresh.hidden_states()[0][0][0, live])
        for env in (A, B):                                                         # the reset forced in between
            env.reset_buf[forced] = True
    assert "unavailable" not in capsys.readouterr().out

    # the graphed policy step: memories from zero on the sims' device step counters
    ga = RecurrentFusedActor(ac, DEV, seed=21, step_counter=A.ll_env._sim.buf["step_counter"], num_envs=n, gru=True)
    gb = RecurrentFusedActor(ac, DEV, seed=21, step_counter=B.ll_env._sim.buf["step_counter"], num_envs=n, gru=True)
    replay = A.make_graphed_policy_step(ga, warmup=3)
    for _ in range(3):
        B.step_policy(gb)
    for k in range(4):
        oa, _, ra, da, _ = replay()
        (cb, mb), (ob, _, rb, db, _) = B.step_policy(gb)
        torch.cuda.synchronize()
        ca, ma = ga.output_buffers(n)
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db) and torch.equal(ca, cb) and torch.equal(ma, mb), k
        _assert_same_state(A, B, k)
        assert _same_memories(ga, gb), k
    assert float(ga.hidden_states()[0][0].abs().max()) > 0.0 and float(ga.hidden_states()[1][0].abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------------------------- DecGamePolicyRunner
from tests.dec_game_fixtures import dec_registered  # noqa: E402,F401


def _dec_runner(reg, root, monkeypatch, ckpt, n=N_GAME, units=64, **runner_keys):
    import legged_games_gym_amd.utils.task_registry as tr_mod
    from legged_games_gym_amd.utils import get_args
    from legged_games_gym_amd.utils.helpers import apply_policy_args
    monkeypatch.setattr(tr_mod, "LEGGED_GYM_ROOT_DIR", str(root))
    env_cfg, train_cfg = reg.get_cfgs("dec_high_level_game")
    env_cfg.env.ll_policy_path = ckpt
    if hasattr(train_cfg.runner, "graphed_rollout"):
        delattr(train_cfg.runner, "graphed_rollout")
    train_cfg.runner.device_rollout = True                                  # runner keys, not config fields: set on this registration only
    for key, value in runner_keys.items():
        setattr(train_cfg.runner, key, value)
    args = get_args(["--task", "dec_high_level_game", "--num_envs", str(n), "--headless", "--sim_device", DEV, "--rl_device", DEV,
                     "--policy_class_name", "ActorCriticRecurrent", "--rnn_type", "gru", "--rnn_hidden_size", str(units)])
    apply_policy_args(train_cfg, args)
    env, _ = reg.make_env("dec_high_level_game", args)
    torch.manual_seed(1234)
    runner, _ = reg.make_dec_alg_runner(env, "dec_high_level_game", args)
    env.ll_env.episode_length_buf[::2] = int(env.ll_env.max_episode_length) - 3 - (torch.arange(0, n, 2, device=DEV) % 41)
    return env, runner, args


def test_dec_runner_trains_two_gru_policies(tmp_path, monkeypatch, dec_registered, capsys):
    from legged_games_gym_amd.rl.recurrent_actor import RecurrentFusedActor
    from tests.test_gpu_game import write_ll_checkpoint
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    try:
        env, runner, _ = _dec_runner(dec_registered, tmp_path / "run", monkeypatch, ckpt, device_gru=True)
        assert runner.recurrent and runner.device_path
        for a in ("pred", "prey"):
            r = runner.runners[a]
            assert isinstance(r._fused, RecurrentFusedActor) and r._fused.gru and r._game_rollout and r._recurrent_rollout
            assert isinstance(r.alg.actor_critic.memory_a.rnn, nn.GRU) and r.alg.actor_critic.memory_a.rnn.hidden_size == 64
        assert env.shared_actor_launch(runner.runners["pred"]._fused, runner.runners["prey"]._fused) is False
        losses = {}
        for a in ("pred", "prey"):
            alg = runner.runners[a].alg

            def update(_update=alg.update, _a=a):
                losses.setdefault(_a, []).append(_update())
                return losses[_a][-1]
            monkeypatch.setattr(alg, "update", update)
        params = lambda a: [p.detach().clone() for p in runner.runners[a].alg.actor_critic.parameters()]
        before = {a: params(a) for a in ("pred", "prey")}
        runner.learn(max_num_evolutions=1, num_learning_iterations=2)            # the predator learns; the prey's actor memory moves as its opponent
        torch.cuda.synchronize()
        carried = runner.runners["prey"]._fused.hidden_states()[0][0].clone()
        assert float(carried.abs().max()) > 0.0 and set(losses) == {"pred"}
        assert all(torch.equal(x, y) for x, y in zip(before["prey"], params("prey")))
        seen = {}
        r = runner.runners["prey"]

        def learn(*x, _learn=r.learn, **k):                                       # what the prey's evolution starts from
            seen["actor"] = r._fused.hidden_states()[0][0].clone()
            return _learn(*x, **k)
        r.learn = learn
        runner.learn(max_num_evolutions=1, num_learning_iterations=2)
        torch.cuda.synchronize()
        assert torch.equal(seen["actor"], carried)                                # the actor memory carried across the evolutions
        assert float(runner.runners["pred"]._fused.hidden_states()[0][0].abs().max()) > 0.0
        assert runner.current_evolution == 2 and {a: len(v) for a, v in losses.items()} == {"pred": 2, "prey": 2}
        assert all(np.isfinite(v) for per in losses.values() for pair in per for v in pair), losses
        assert all(bool(torch.isfinite(p).all()) for a in ("pred", "prey") for p in runner.runners[a].alg.actor_critic.parameters())
        assert any(not torch.equal(x, y) for x, y in zip(before["prey"], params("prey")))
        ac = runner.runners["pred"].alg.actor_critic
        assert not torch.equal(before["pred"][[n for n, _ in ac.named_parameters()].index("memory_a.rnn.weight_hh_l0")], ac.memory_a.rnn.weight_hh_l0)
        said = capsys.readouterr().out
        lines = [l for l in said.splitlines() if "unavailable" in l]
        assert len(lines) == 1 and "GRU memory" in lines[0] and "lg_lstm_actor_act x 2 + lg_dec_game_pre + lg_policy_act" in lines[0], said
    finally:
        _, train_cfg = dec_registered.get_cfgs("dec_high_level_game")              # the registered object is shared: leave it as it was found
        for obj, keys in ((train_cfg.runner, ("device_rollout", "policy_class_name", "device_gru")), (train_cfg.policy, ("rnn_hidden_size", "rnn_type"))):
            for key in keys:
                if key in vars(obj):
                    delattr(obj, key)
