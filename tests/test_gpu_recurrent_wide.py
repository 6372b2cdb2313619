"""The wide LSTM cell and actor on the GPU (``lg_lstm_wide_*``, include/legged_recurrent_wide.h: k_lstm_wide_cell, k_lstm_wide_pack,
k_lstm_wide_actor, k_lstm_wide_actor_pack): memories of 288 .. 512 units against the float64 restatements of ``tests/recurrent_ref.py``,
bit for bit against the 256-unit kernels where both take a shape, the existing edge families (saturated gates, stale state of reset rows,
aliasing, capture, ``load_device``) at 512 units, and ``RecurrentFusedActor(wide=True)`` through both runners with the key ``wide_memory``.

The bar is ``TOL = 2e-5`` of the output scale, the one of ``tests/test_gpu_recurrent.py``.  The float32 ``nn.LSTM`` stays within 1.2e-6 (h) and
1.8e-6 (c) of float64 on a CPU at (1, 288), (3, 512), (48, 512), (235, 512), (256, 512), (256, 480) with 33 rows, default weights and
weights x 3: under 0.1 of the bar."""
import copy
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests.noise_check import check_noise
from tests.recurrent_ref import actor_forward64, actor_params64, lstm_params64, lstm_step64, saturating_bias

pytestmark = pytest.mark.gpu
TOL = 2e-5
DEV = "cuda:0"
EXTRA = 5                    # NaN guard rows behind row N of every input and output


def _rnn(I, H, seed, gain=1.0):
    torch.manual_seed(seed)
    rnn = nn.LSTM(I, H).to(DEV)
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
    from legged_games_gym_amd.rl.recurrent_actor import DeviceLstm, lstm_step
    wide = capi.load_lstm_wide_library()
    return (lambda rnn: DeviceLstm(rnn, DEV, wide=True)), lstm_step, wide


def _narrow():
    from legged_games_gym_amd import capi
    from legged_games_gym_amd.rl.recurrent_actor import DeviceLstm
    return (lambda rnn: DeviceLstm(rnn, DEV)), capi.load_library()


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _np64(t):
    return t.detach().cpu().double().numpy()


def _one(lstm_step, lib, cell, x, h, c, reset=None, role="actor"):
    """One launch of one role into fresh guarded outputs; returns ``(h_out, c_out)``."""
    n, H = h.shape
    (fh, ho), (fc, co) = _padded(n, H), _padded(n, H)
    if role == "actor":
        lstm_step(lib, cell, None, x, None, reset, (h, c), (ho, co), None, None, n, _stream())
    else:
        lstm_step(lib, None, cell, None, x, reset, None, None, (h, c), (ho, co), n, _stream())
    torch.cuda.synchronize()
    assert torch.isnan(fh[n:]).all() and torch.isnan(fc[n:]).all()
    return ho, co


# ---------------------------------------------------------------------------------------------------------------- the cell against float64
# every hidden size (288: the second group is one wave; 480: seven waves; 512), every input count (1; 3: odd K, the pad row; 256: the
# largest LDS block) and every N (one row; one short of, exactly and one past a block; three blocks) at least twice
CELL_CASES = [(1, 288, 1), (3, 512, 33), (48, 320, 31), (235, 512, 65), (256, 512, 32), (256, 480, 33), (3, 288, 65), (48, 480, 1), (235, 320, 32),
              (1, 512, 31)]


@pytest.mark.parametrize("I,H,N", CELL_CASES)
def test_one_step_matches_float64(I, H, N):
    """Both roles in one launch (the critic with another num_in), each role alone; reset null and mixed.  Inputs and outputs sit between NaN
    guard rows."""
    make, lstm_step, lib = _cells()
    Ic = I + 7 if I + 7 <= 256 else I - 7
    rnn_a, rnn_c = _rnn(I, H, 1), _rnn(Ic, H, 2)
    la, lc = make(rnn_a), make(rnn_c)
    gen = torch.Generator().manual_seed(I * 1000 + N)
    xa, xc = _uniform(gen, N, I), _uniform(gen, N, Ic)
    ha, ca, hc, cc = (_uniform(gen, N, H, 1.0) for _ in range(4))
    mixed = (torch.arange(N) % 3 == 0).to(torch.uint8).to(DEV)
    pa, pc = lstm_params64(rnn_a), lstm_params64(rnn_c)
    worst = 0.0
    for name, reset in (("null", None), ("mixed", mixed)):
        r = None if reset is None else reset.cpu().numpy()
        want_a = lstm_step64(pa, _np64(xa), _np64(ha), _np64(ca), r)
        want_c = lstm_step64(pc, _np64(xc), _np64(hc), _np64(cc), r)
        for roles in ("both", "actor", "critic"):
            full, outs = zip(*[_padded(N, H) for _ in range(4)])
            lstm_step(lib, la if roles != "critic" else None, lc if roles != "actor" else None, xa, xc, reset, (ha, ca), (outs[0], outs[1]), (hc, cc),
                      (outs[2], outs[3]), N, _stream())
            torch.cuda.synchronize()
            got = [_np64(o) for o in outs]
            for present, pair, want, who in ((roles != "critic", got[:2], want_a, "actor"), (roles != "actor", got[2:], want_c, "critic")):
                if present:
                    err = max(np.abs(pair[0] - want[0]).max(), np.abs(pair[1] - want[1]).max())
                    worst = max(worst, err)
                    assert np.isfinite(pair[0]).all() and np.isfinite(pair[1]).all()
                    assert err < TOL, (name, roles, who, err)
                else:
                    assert np.isnan(pair[0]).all() and np.isnan(pair[1]).all()      # an absent role writes nothing
            for f in full:
                assert torch.isnan(f[N:]).all()                                    # the sentinels behind row N are intact
    print(f"[observed] wide cell ({I},{H},{N}): worst err {worst:.3e} = {worst / TOL:.3f} of the bar")


def test_one_step_with_weights_times_three_matches_float64():
    make, lstm_step, lib = _cells()
    I, H, N = 48, 512, 33
    rnn = _rnn(I, H, 3, gain=3.0)
    cell = make(rnn)
    gen = torch.Generator().manual_seed(5)
    x, h, c = _uniform(gen, N, I), _uniform(gen, N, H, 1.0), _uniform(gen, N, H, 1.0)
    ho, co = _one(lstm_step, lib, cell, x, h, c)
    want = lstm_step64(lstm_params64(rnn), _np64(x), _np64(h), _np64(c))
    err = max(np.abs(_np64(ho) - want[0]).max(), np.abs(_np64(co) - want[1]).max())
    print(f"[observed] wide cell weights x 3 ({I},{H},{N}): err {err:.3e} = {err / TOL:.3f} of the bar")
    assert err < TOL


@pytest.mark.parametrize("Ha,Hc", [(512, 64), (64, 512)])
def test_roles_of_different_hidden_size_in_one_launch(Ha, Hc):
    """The narrower role has no second unit group: its workgroups are fewer and their surplus waves only stage."""
    make, lstm_step, lib = _cells()
    I, Ic, N = 19, 26, 37
    rnn_a, rnn_c = _rnn(I, Ha, 1), _rnn(Ic, Hc, 2)
    la, lc = make(rnn_a), make(rnn_c)
    gen = torch.Generator().manual_seed(Ha)
    xa, xc = _uniform(gen, N, I), _uniform(gen, N, Ic)
    ha, ca = (_uniform(gen, N, Ha, 1.0) for _ in range(2))
    hc, cc = (_uniform(gen, N, Hc, 1.0) for _ in range(2))
    reset = (torch.arange(N) % 3 == 0).to(torch.uint8).to(DEV)
    r = reset.cpu().numpy()
    want = (lstm_step64(lstm_params64(rnn_a), _np64(xa), _np64(ha), _np64(ca), r) + lstm_step64(lstm_params64(rnn_c), _np64(xc), _np64(hc), _np64(cc), r))
    full, outs = zip(*[_padded(N, H) for H in (Ha, Ha, Hc, Hc)])
    lstm_step(lib, la, lc, xa, xc, reset, (ha, ca), (outs[0], outs[1]), (hc, cc), (outs[2], outs[3]), N, _stream())
    torch.cuda.synchronize()
    for i, (o, w) in enumerate(zip(outs, want)):
        err = np.abs(_np64(o) - w).max()
        print(f"[observed] hidden ({Ha},{Hc}) output {i}: err {err:.3e}")
        assert err < TOL, (i, err)
    for f in full:
        assert torch.isnan(f[N:]).all()


# ---------------------------------------------------------------------------------------------------------------- bit for bit
@pytest.mark.parametrize("I,H", [(19, 32), (235, 160), (48, 256)])
def test_the_wide_cell_equals_the_256_unit_cell_bit_for_bit(I, H):
    """A unit's chain does not depend on the launch: at a width both kernels take, ``lg_lstm_wide_step`` = ``lg_lstm_step``."""
    make, lstm_step, wide = _cells()
    make_n, main = _narrow()
    N, Ic = 65, I + 7
    rnn_a, rnn_c = _rnn(I, H, 1), _rnn(Ic, H, 2)
    gen = torch.Generator().manual_seed(H)
    xa, xc = _uniform(gen, N, I), _uniform(gen, N, Ic)
    ha, ca, hc, cc = (_uniform(gen, N, H, 1.0) for _ in range(4))
    reset = (torch.arange(N) % 4 == 1).to(torch.uint8).to(DEV)
    results = []
    for mk, lib in ((make, wide), (make_n, main)):
        la, lc = mk(rnn_a), mk(rnn_c)
        outs = [torch.full((N, H), float("nan"), device=DEV) for _ in range(4)]
        lstm_step(lib, la, lc, xa, xc, reset, (ha, ca), (outs[0], outs[1]), (hc, cc), (outs[2], outs[3]), N, _stream())
        torch.cuda.synchronize()
        results.append(outs)
    for i, (a, b) in enumerate(zip(*results)):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), i


def test_a_block_diagonal_512_unit_cell_equals_its_two_256_unit_halves_bit_for_bit():
    """``W_hh`` couples units 0 .. 255 only to ``h[:256]`` and units 256 .. 511 only to ``h[256:]``; every other weight of a half comes from a
    256-unit cell.  A zero product leaves an ``fmaf`` chain unchanged (the accumulators start from random non-zero biases: none is -0), and
    256 is even, so a half's k-steps pair the same operands: each half equals ``lg_lstm_step`` of its cell.  A dropped, repeated or swapped
    unit group shows as a bit difference."""
    make, lstm_step, wide = _cells()
    make_n, main = _narrow()
    I, N, h = 47, 65, 256                                       # odd K: a k-step straddles x and h, in the halves and in the whole alike
    halves = [_rnn(I, h, 11), _rnn(I, h, 12)]
    big = _rnn(I, 2 * h, 13)
    with torch.no_grad():
        big.weight_hh_l0.zero_()
        for g in range(4):
            for j, half in enumerate(halves):
                rows = slice(g * 2 * h + j * h, g * 2 * h + (j + 1) * h)
                big.weight_ih_l0[rows] = half.weight_ih_l0[g * h:(g + 1) * h]
                big.weight_hh_l0[rows, j * h:(j + 1) * h] = half.weight_hh_l0[g * h:(g + 1) * h]
                big.bias_ih_l0[rows] = half.bias_ih_l0[g * h:(g + 1) * h]
                big.bias_hh_l0[rows] = half.bias_hh_l0[g * h:(g + 1) * h]
        assert all(float((p.bias_ih_l0 + p.bias_hh_l0).abs().min()) > 0.0 for p in halves)
    gen = torch.Generator().manual_seed(17)
    x = _uniform(gen, N, I)
    hs, cs = [_uniform(gen, N, h, 1.0) for _ in range(2)], [_uniform(gen, N, h, 1.0) for _ in range(2)]
    reset = (torch.arange(N) % 5 == 2).to(torch.uint8).to(DEV)
    ho, co = _one(lstm_step, wide, make(big), x, _guarded(torch.cat(hs, 1)), _guarded(torch.cat(cs, 1)), reset)
    for j, half in enumerate(halves):
        want_h, want_c = _one(lstm_step, main, make_n(half), x, hs[j], cs[j], reset)
        assert torch.equal(ho[:, j * h:(j + 1) * h], want_h) and torch.equal(co[:, j * h:(j + 1) * h], want_c), j
    assert not torch.equal(ho[:, :h], ho[:, h:])


@pytest.mark.parametrize("I,H", [(3, 512), (48, 288)])
def test_exact_placement_of_every_weight_column(I, H):
    """One-hot ``x`` (then one-hot ``h``) at column k with zero biases and a zero state: the outputs follow from column k of ``W_ih``
    (``W_hh``) alone.  Row n of the batch carries the n-th tested column."""
    make, lstm_step, lib = _cells()
    rnn = _rnn(I, H, 3)
    with torch.no_grad():
        rnn.bias_ih_l0.zero_(); rnn.bias_hh_l0.zero_()
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
        c = torch.zeros(N, H, device=DEV)
        h_out, c_out = _one(lstm_step, lib, cell, x, h, c)
        W64 = _np64(W)
        for n, k in enumerate(ks):
            col = W64[:, k].reshape(4, H)
            c_want = sig(col[0]) * np.tanh(col[2])
            h_want = sig(col[3]) * np.tanh(c_want)
            assert np.abs(_np64(c_out[n]) - c_want).max() < TOL, (which, k)
            assert np.abs(_np64(h_out[n]) - h_want).max() < TOL, (which, k)


# ---------------------------------------------------------------------------------------------------------------- edges at 512 units
def test_saturated_gates_stay_finite_and_exact():
    """``saturating_bias`` at 512 units: sigma / tanh come out as exactly 0 / 1 / -1, never NaN; 24 steps within the bar of the scales of
    h and c."""
    I, H, N, T = 19, 512, 9, 24
    make, lstm_step, lib = _cells()
    rnn = _rnn(I, H, 6)
    with torch.no_grad():
        rnn.bias_ih_l0.add_(torch.from_numpy(saturating_bias(H)).float().to(DEV))
    cell = make(rnn)
    gen = torch.Generator().manual_seed(13)
    xs = [_uniform(gen, N, I) for _ in range(T)]
    p = lstm_params64(rnn)
    st = [(torch.zeros(N, H, device=DEV), torch.zeros(N, H, device=DEV)) for _ in range(2)]
    h, c = np.zeros((N, H)), np.zeros((N, H))
    err_h = err_c = scale_h = scale_c = 0.0
    for t in range(T):
        lstm_step(lib, cell, None, xs[t], None, None, st[t & 1], st[1 - (t & 1)], None, None, N, _stream())
        torch.cuda.synchronize()
        got_h, got_c = st[1 - (t & 1)]
        h, c = lstm_step64(p, _np64(xs[t]), h, c)
        assert bool(torch.isfinite(got_h).all()) and bool(torch.isfinite(got_c).all()), t
        assert bool((got_h[:, 4::8] == 0.0).all()), t            # output gate at -1e4: sigma is exactly 0
        assert bool((got_c[:, 2::8] == 1.0).all()), t            # i at +1e4, f at -1e4 and g at +30: c = 0 c + 1 * 1
        err_h, err_c = max(err_h, np.abs(_np64(got_h) - h).max()), max(err_c, np.abs(_np64(got_c) - c).max())
        scale_h, scale_c = max(scale_h, np.abs(h).max()), max(scale_c, np.abs(c).max())
    print(f"[observed] wide saturated gates: h err {err_h:.3e} (max |h| {scale_h:.3f}), c err {err_c:.3e} (max |c| {scale_c:.3f})")
    assert scale_c > 10.0                                        # the pinned-open forget gates did accumulate
    assert err_h < TOL * max(1.0, scale_h) and err_c < TOL * max(1.0, scale_c), (err_h, err_c)


def test_a_reset_row_ignores_its_stale_state():
    """Flag bytes 1, 2 and 255 start a row from zeros by selection: NaN and +-Inf in its ``h_in`` / ``c_in`` reach no output, and the outputs
    are bit-equal to the run with zeros in those places (both roles, 512 units)."""
    make, lstm_step, lib = _cells()
    I, Ic, H, N = 19, 26, 512, 37
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
        poisoned[3, 1], poisoned[6, H - 1], poisoned[9, 300] = float("inf"), float("-inf"), float("inf")
        return _guarded(poisoned), _guarded(clean)

    xa, xc = _uniform(gen, N, I), _uniform(gen, N, Ic)
    states = [state() for _ in range(4)]
    results = []
    for k in (0, 1):
        ha, ca, hc, cc = (s[k] for s in states)
        full, outs = zip(*[_padded(N, H) for _ in range(4)])
        lstm_step(lib, la, lc, xa, xc, flags, (ha, ca), (outs[0], outs[1]), (hc, cc), (outs[2], outs[3]), N, _stream())
        torch.cuda.synchronize()
        for f in full:
            assert torch.isnan(f[N:]).all()
        results.append([o.clone() for o in outs])
    for got, want in zip(*results):
        assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
    want_c = lstm_step64(lstm_params64(rnn_c), _np64(xc), _np64(states[2][1]), _np64(states[3][1]), flagged.numpy())
    assert np.abs(_np64(results[0][2]) - want_c[0]).max() < TOL and np.abs(_np64(results[0][3]) - want_c[1]).max() < TOL


def test_aliasing_is_refused():
    make, lstm_step, lib = _cells()
    I, H, N = 19, 512, 33
    cell = make(_rnn(I, H, 1))
    x, h, c, o = (torch.zeros(N, w, device=DEV) for w in (I, H, H, H))
    for outs in ((h, o), (o, c), (c, o), (o, h), (o, o)):
        rc = lib.lg_lstm_wide_step(cell.handle, None, x.data_ptr(), None, None, h.data_ptr(), c.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(),
                                   None, None, None, None, N, _stream())
        assert rc == -2 and b"alias" in lib.lg_lstm_wide_last_error()
        rc = lib.lg_lstm_wide_step(None, cell.handle, None, x.data_ptr(), None, None, None, None, None, h.data_ptr(), c.data_ptr(), outs[0].data_ptr(),
                                   outs[1].data_ptr(), N, _stream())
        assert rc == -2 and b"alias" in lib.lg_lstm_wide_last_error()
    torch.cuda.synchronize()
    assert float(o.abs().max()) == 0.0 and float(h.abs().max()) == 0.0


def _run_24(cell, lstm_step, lib, xs, resets, N, H, graphed):
    """24 steps on ping-ponged state buffers from a zero state; returns the [24, N, H] outputs and the last c."""
    T = xs.shape[0]
    st = [(torch.zeros(N, H, device=DEV), torch.zeros(N, H, device=DEV)) for _ in range(2)]
    hs = torch.empty(T, N, H, device=DEV)
    x_in, r_in = torch.empty_like(xs[:2]), torch.empty_like(resets[:2])

    def two(src_x, src_r, out):
        for j in range(2):
            lstm_step(lib, cell, None, src_x[j], None, src_r[j], st[j], st[1 - j], None, None, N, _stream())
            out[j].copy_(st[1 - j][0])

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
    return hs, st[0][1].clone()


def test_24_steps_replay_bit_identically():
    I, H, N, T = 19, 512, 70, 24
    make, lstm_step, lib = _cells()
    cell = make(_rnn(I, H, 4))
    gen = torch.Generator().manual_seed(11)
    xs = (torch.rand(T, N, I, generator=gen) * 6.0 - 3.0).to(DEV)
    resets = (torch.rand(T, N, generator=gen) < 0.1).to(torch.uint8).to(DEV)
    a, ca = _run_24(cell, lstm_step, lib, xs, resets, N, H, False)
    b, cb = _run_24(cell, lstm_step, lib, xs, resets, N, H, False)
    assert bool(torch.isfinite(a).all()) and float(a[-1].abs().max()) > 0.0
    assert torch.equal(a, b) and torch.equal(ca, cb)
    g, cg = _run_24(cell, lstm_step, lib, xs, resets, N, H, True)
    assert torch.equal(a, g) and torch.equal(ca, cg)


def test_load_device_equals_create_and_the_next_launch_sees_new_parameters():
    I, H, N = 48, 512, 37
    make, lstm_step, lib = _cells()
    rnn = _rnn(I, H, 5)
    first = make(rnn)
    gen = torch.Generator().manual_seed(3)
    x, h, c = _uniform(gen, N, I), _uniform(gen, N, H, 1.0), _uniform(gen, N, H, 1.0)
    before = _one(lstm_step, lib, first, x, h, c)
    with torch.no_grad():
        for prm in rnn.parameters():
            prm.add_(0.05 * torch.randn_like(prm))
    stale = _one(lstm_step, lib, first, x, h, c)                 # the handle owns its operands: the module moved, the handle did not
    assert torch.equal(stale[0], before[0]) and torch.equal(stale[1], before[1])
    fresh = make(rnn)                                            # lg_lstm_wide_create from the host copies of the new weights
    first.load_device()                                          # lg_lstm_wide_load_device from the CUDA parameters
    a, b = _one(lstm_step, lib, first, x, h, c), _one(lstm_step, lib, fresh, x, h, c)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], before[0])
    want = lstm_step64(lstm_params64(rnn), _np64(x), _np64(h), _np64(c))
    assert np.abs(_np64(a[0]) - want[0]).max() < TOL and np.abs(_np64(a[1]) - want[1]).max() < TOL


# ---------------------------------------------------------------------------------------------------------------- the actor
# (dims[0]; hidden widths; actions; N)
ACTOR_CASES = [
    (512, (32, 32, 32), 1, 1),          # the widest input on the narrowest layers
    (512, (512, 256, 128), 12, 33),     # the reference's policy behind a 512-unit memory
    (288, (96, 160, 224), 6, 33),       # tile counts 3, 5, 7 that the wave count does not divide; the games' 6 actions
    (512, (512, 512, 512), 16, 64),     # every buffer at full width; N an exact multiple of 32
    (512, (32, 32, 32), 1, 64),
    (288, (96, 160, 224), 6, 1),
]


def _policy(H, hidden, nA, seed, gain=1.0):
    """What ``DeviceLstmActor`` reads of an actor-critic: ``.actor`` (Linear / ELU x 3 / Linear) and ``.std``."""
    torch.manual_seed(seed)
    dims = (H,) + tuple(hidden) + (nA,)
    mods = []
    for i in range(4):
        lin = nn.Linear(dims[i], dims[i + 1], device=DEV)
        with torch.no_grad():
            lin.weight.mul_(gain)
            lin.bias.uniform_(-1.0, 1.0)
        mods += [lin] + ([nn.ELU()] if i < 3 else [])
    return types.SimpleNamespace(actor=nn.Sequential(*mods), std=torch.linspace(0.3, 1.4, nA).to(DEV))


def _device_actor(policy, seed=5, step_counter=None, wide=True):
    from legged_games_gym_amd.rl.recurrent_actor import DeviceLstmActor
    return DeviceLstmActor(policy, DEV, seed=seed, step_counter=step_counter, wide=wide)


def _memory_output(N, H, seed):
    return _guarded(torch.rand(N, H, generator=torch.Generator().manual_seed(seed)) * 2.0 - 1.0)


def _act(da, h, N, seed, step, counter=None, deterministic=False, with_mean=True):
    """One raw ``lg_lstm_wide_actor_act`` (``lg_lstm_actor_act`` for a narrow handle); returns the FULL ``actions`` / ``mean`` buffers."""
    nA = da.num_actions
    actions = torch.full((N + EXTRA, nA), float("nan"), device=DEV)
    mean = torch.full((N + EXTRA, nA), float("nan"), device=DEV) if with_mean else None
    fn = da.lib.lg_lstm_wide_actor_act if da.wide else da.lib.lg_lstm_actor_act
    rc = fn(da.handle, h.data_ptr(), actions.data_ptr(), mean.data_ptr() if with_mean else None, N, seed, step,
            counter.data_ptr() if counter is not None else None, int(deterministic), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return actions, mean


@pytest.mark.parametrize("gain", [1.0, 3.0], ids=["default_weights", "weights_x3"])
@pytest.mark.parametrize("H,hidden,nA,N", ACTOR_CASES, ids=[f"{c[0]}-{'-'.join(map(str, c[1]))}-{c[2]}_N{c[3]}" for c in ACTOR_CASES])
def test_actor_means_match_float64_and_the_flags_do_what_they_say(H, hidden, nA, N, gain):
    policy = _policy(H, hidden, nA, seed=H + N, gain=gain)
    da = _device_actor(policy)
    h = _memory_output(N, H, seed=N)
    seed, step = 5, 3
    actions, mean = _act(da, h, N, seed, step)
    want = actor_forward64(*actor_params64(policy.actor), _np64(h))
    scale = max(1.0, float(np.abs(want).max()))
    got = _np64(mean[:N])
    assert np.isfinite(got).all() and bool(torch.isfinite(actions[:N]).all())      # the NaN rows behind h stayed out
    err = float(np.abs(got - want).max())
    print(f"[observed] wide actor {H}-{'-'.join(map(str, hidden))}-{nA} N={N} gain {gain}: mean err {err:.3e}, scale {scale:.3f}, "
          f"{err / (TOL * scale):.3f} of the bar")
    assert err < TOL * scale, (err, scale)
    assert bool(torch.isnan(actions[N:]).all()) and bool(torch.isnan(mean[N:]).all())      # the sentinels behind row N are intact
    assert float((actions[:N] - mean[:N]).abs().max()) > 0.0

    det_actions, det_mean = _act(da, h, N, seed, step, deterministic=True)
    assert torch.equal(det_actions[:N], det_mean[:N]) and torch.equal(det_mean[:N], mean[:N])
    no_mean, _ = _act(da, h, N, seed, step, with_mean=False)                     # mean = NULL: accepted, the same actions
    assert torch.equal(no_mean[:N], actions[:N]) and bool(torch.isnan(no_mean[N:]).all())
    a_w, m_w = (t.clone() for t in da.act_with_mean(h))                          # the wrapper: its first call is host step 1
    torch.cuda.synchronize()
    a_1, m_1 = _act(da, h, N, seed, 1)
    assert torch.equal(a_w, a_1[:N]) and torch.equal(m_w, m_1[:N]) and torch.equal(m_w, mean[:N])


@pytest.mark.parametrize("H,hidden,nA", [(64, (128, 64, 32), 12), (256, (512, 256, 128), 13)])
def test_the_wide_actor_equals_the_256_unit_actor_bit_for_bit(H, hidden, nA):
    """An output tile is one k-ordered chain on one wave, whichever wave: 8 waves with 16 k-steps ahead give the bits of 4 waves with 4."""
    policy = _policy(H, hidden, nA, seed=3)
    wide, narrow = _device_actor(policy), _device_actor(policy, wide=False)
    for N in (1, 33, 64):
        h = _memory_output(N, H, seed=N)
        for det in (False, True):
            (aw, mw), (an, mn) = _act(wide, h, N, 5, 7, deterministic=det), _act(narrow, h, N, 5, 7, deterministic=det)
            assert torch.equal(aw[:N], an[:N]) and torch.equal(mw[:N], mn[:N]), (N, det)


@pytest.mark.parametrize("nA", [1, 6, 13, 16])
def test_actor_noise_is_the_reference_stream(nA):
    """``actions - mean`` is ``std * eps`` of the independent Philox reference for (seed; env, step), under the bars of tests/noise_check.py:
    a host step, one above 2^32, and ``step = -1`` with a device counter holding c (the stream of step c + 1; the counter stays)."""
    H, hidden, N, seed = 512, (32, 32, 32), 37, 9
    policy = _policy(H, hidden, nA, seed=nA)
    da = _device_actor(policy, seed=seed)
    h = _memory_output(N, H, seed=nA)
    std = _np64(policy.std)
    report = {}
    for step in (41, 2 ** 32 + 4242):
        actions, mean = _act(da, h, N, seed, step)
        check_noise(actions[:N].cpu().numpy(), mean[:N].cpu().numpy(), std, seed, step, report)
        assert bool(torch.isnan(actions[N:]).all()) and bool(torch.isnan(mean[N:]).all())
    c = 776
    counter = torch.tensor([c], dtype=torch.int64, device=DEV)
    actions, mean = _act(da, h, N, seed, -1, counter=counter)
    check_noise(actions[:N].cpu().numpy(), mean[:N].cpu().numpy(), std, seed, c + 1, report)
    assert int(counter[0]) == c
    by_host, _ = _act(da, h, N, seed, c + 1)
    assert torch.equal(by_host[:N], actions[:N])
    a_w, m_w = _device_actor(policy, seed=seed, step_counter=counter).act_with_mean(h)      # the wrapper with the env's device counter
    torch.cuda.synchronize()
    assert torch.equal(a_w, actions[:N]) and torch.equal(m_w, mean[:N]) and int(counter[0]) == c
    print(f"[observed] wide actor noise nA={nA}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(report.items())))


def test_actor_sync_device_equals_a_fresh_handle():
    H, hidden, nA, N = 512, (512, 256, 128), 12, 33
    policy = _policy(H, hidden, nA, seed=17)
    first = _device_actor(policy)
    h = _memory_output(N, H, seed=2)
    before, _ = _act(first, h, N, 5, 7)
    with torch.no_grad():
        for prm in policy.actor.parameters():
            prm.add_(0.05 * torch.randn_like(prm))
        policy.std.mul_(0.7)
    first.sync_device()
    fresh = _device_actor(policy)
    (a_first, m_first), (a_fresh, m_fresh) = _act(first, h, N, 5, 7), _act(fresh, h, N, 5, 7)
    assert torch.equal(a_first[:N], a_fresh[:N]) and torch.equal(m_first[:N], m_fresh[:N]) and not torch.equal(a_first[:N], before[:N])
    want = actor_forward64(*actor_params64(policy.actor), _np64(h))
    assert float(np.abs(_np64(m_first[:N]) - want).max()) < TOL * max(1.0, float(np.abs(want).max()))


# ---------------------------------------------------------------------------------------------------------------- RecurrentFusedActor(wide=True)
def test_the_reference_configuration_through_the_wrapper():
    """The reference's commented recurrent setting on the rough task: 235 observations, 512 units per memory, the 512-512-256-128-12 actor.
    Four steps with dones (one env done twice in a row) against a float64 CPU copy of the module; ``peek_critic`` leaves the carried state."""
    from legged_games_gym_amd import capi
    from legged_games_gym_amd.rl import ActorCriticRecurrent
    from legged_games_gym_amd.rl.recurrent_actor import RecurrentFusedActor
    N, T = 33, 4
    torch.manual_seed(8)
    ac = ActorCriticRecurrent(235, 235, 12, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128], rnn_hidden_size=512).to(DEV)
    assert ac.memory_a.rnn.hidden_size == 512 and ac.actor[0].in_features == 512
    ac64 = copy.deepcopy(ac).double().cpu()
    with pytest.raises(ValueError, match="up to 256"):
        RecurrentFusedActor(ac, DEV, seed=5)
    rfa = RecurrentFusedActor(ac, DEV, seed=5, wide=True)
    assert rfa.wide is True and rfa.recurrent is True and rfa.lstm_a.wide and rfa.lstm_c.wide and rfa.fused.wide
    assert rfa.cell_lib is capi.load_lstm_wide_library() and rfa.lib is capi.load_library() and rfa.num_actions == 12 and rfa.handle is rfa.fused.handle
    gen = torch.Generator().manual_seed(10)
    obs = (torch.rand(T, N, 235, generator=gen) * 6.0 - 3.0).to(DEV)
    dones = torch.rand(T, N, generator=gen) < 0.25
    dones[:, 32] = torch.tensor([False, True, True, False])      # the single row of the second row block: done twice in a row
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
            e_m, e_h = np.abs(_np64(mean) - want_mean).max(), np.abs(_np64(h_c) - want_hc).max()
            s_m, s_h = max(1.0, np.abs(want_mean).max()), max(1.0, np.abs(want_hc).max())
            print(f"[observed] wide wrapper step {t}: mean err {e_m:.3e} (scale {s_m:.3f}), critic memory err {e_h:.3e} (scale {s_h:.3f})")
            assert e_m < TOL * s_m and e_h < TOL * s_h, (t, e_m, e_h)
        before = [x.clone() for pair in (rfa.state_a[rfa._flip], rfa.state_c[rfa._flip]) for x in pair]
        peek = rfa.peek_critic(obs[0], dones[T - 1].to(DEV)).clone()
        torch.cuda.synchronize()
        after = [x for pair in (rfa.state_a[rfa._flip], rfa.state_c[rfa._flip]) for x in pair]
        assert all(torch.equal(a, b) for a, b in zip(before, after))
        want_peek = ac64.memory_c(obs[0].cpu().double()).squeeze(0).numpy()      # (ac64 was reset with dones[T - 1] above)
        assert np.abs(_np64(peek) - want_peek).max() < TOL * max(1.0, np.abs(want_peek).max())
        # publish_states: the torch memories start from the device state
        rfa.publish_states()
        (ha, ca), (hc, cc) = rfa.hidden_states()
        assert torch.equal(ac.memory_a.hidden_states[0], ha) and torch.equal(ac.memory_c.hidden_states[1], cc)
        # an actor-only step keeps both critic slots current; hold_slot reads from the same slot again
        flip = rfa._flip
        rfa.step_memories(obs[0])
        assert rfa._flip == 1 - flip and all(torch.equal(a, b) for a, b in zip(rfa.state_c[0], rfa.state_c[1]))
        rfa.hold_slot()
        assert rfa._flip == flip and all(torch.equal(a, b) for a, b in zip(rfa.state_a[0], rfa.state_a[1]))


def test_wide_with_256_units_builds_nothing_wide():
    from legged_games_gym_amd import capi
    from legged_games_gym_amd.rl import ActorCriticRecurrent
    from legged_games_gym_amd.rl.recurrent_actor import RecurrentFusedActor
    torch.manual_seed(8)
    ac = ActorCriticRecurrent(48, 48, 12, actor_hidden_dims=[128, 64, 32], critic_hidden_dims=[128, 64, 32], rnn_hidden_size=256).to(DEV)
    a, b = RecurrentFusedActor(ac, DEV, seed=5, wide=True), RecurrentFusedActor(ac, DEV, seed=5)
    assert a.wide is False and a.lib is capi.load_library() and a.cell_lib is a.lib and not a.lstm_a.wide and not a.fused.wide
    obs = (torch.rand(33, 48, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(DEV)
    ra, rb = a.act_with_mean(obs, obs), b.act_with_mean(obs, obs)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(ra, rb))


# ---------------------------------------------------------------------------------------------------------------- OnPolicyRunner
def _runner(monkeypatch, hidden=512, graphed=True, steps=24, **runner_keys):
    from legged_games_gym_amd.envs import task_registry
    from legged_games_gym_amd.utils import get_args
    from legged_games_gym_amd.utils.helpers import apply_policy_args
    _, train_cfg = task_registry.get_cfgs("anymal_c_flat")
    args = get_args(["--task", "anymal_c_flat", "--num_envs", "64", "--headless", "--sim_device", DEV, "--rl_device", DEV,
                     "--policy_class_name", "ActorCriticRecurrent", "--rnn_hidden_size", str(hidden)])
    for obj, name in ((train_cfg.runner, "policy_class_name"), (train_cfg.runner, "num_steps_per_env"), (train_cfg.runner, "max_iterations"),
                      (train_cfg.policy, "rnn_hidden_size")):      # the registered cfg is shared: put every field back afterwards
        monkeypatch.setattr(obj, name, getattr(obj, name, None), raising=False)
    train_cfg.runner.num_steps_per_env = steps
    apply_policy_args(train_cfg, args)
    for name, value in runner_keys.items():
        monkeypatch.setattr(train_cfg.runner, name, value, raising=False)
    env, _ = task_registry.make_env("anymal_c_flat", args)
    runner, _ = task_registry.make_alg_runner(env, "anymal_c_flat", args, log_root=None)
    runner.cfg["graphed_rollout"] = graphed
    n = env.num_envs                                         # time-outs inside the first rollouts
    env.episode_length_buf[::2] = int(env.max_episode_length) - 2 - (torch.arange(0, n, 2, device=env.device) % 11)
    return env, runner


def test_runner_device_rollout_at_512_units_eager_and_graphed(monkeypatch, capsys):
    from legged_games_gym_amd.rl.recurrent_actor import RecurrentFusedActor
    from tests.test_gpu_recurrent import _check_storage_against_batch_mode, _snapshot, _stats
    env_g, run_g = _runner(monkeypatch, graphed=True, wide_memory=True)
    assert isinstance(run_g._fused, RecurrentFusedActor) and run_g._fused.wide and run_g._recurrent_rollout and run_g.num_steps_per_env == 24
    assert run_g.alg.actor_critic.memory_a.rnn.hidden_size == 512
    built = run_g._try_build_graphed_rollout()               # one eager warm-up rollout, then the capture
    assert built is not None, capsys.readouterr().out
    built[0].replay()
    run_g.alg.storage.step = run_g.num_steps_per_env
    torch.cuda.synchronize()
    assert float(run_g.alg.storage.initial_hidden_a[0].abs().max()) > 0.0      # the second rollout: a carried-in state
    _check_storage_against_batch_mode(run_g, "wide, graphed")
    snap_g = _snapshot(run_g.alg.storage)

    env_e, run_e = _runner(monkeypatch, graphed=False, wide_memory=True)
    stats = _stats(run_e)
    with torch.inference_mode():
        run_e._rollout_steps(stats)                          # what the warm-up of the graphed runner did
        run_e.alg.storage.clear()
        run_e._rollout_steps(stats)
    torch.cuda.synchronize()
    _check_storage_against_batch_mode(run_e, "wide, eager, second rollout")
    for i, (a, b) in enumerate(zip(snap_g, _snapshot(run_e.alg.storage))):
        assert torch.equal(a, b), f"storage tensor {i} differs between the graph replay and the eager rollout"

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


def test_runner_without_the_key_says_what_it_says_today(monkeypatch, capsys):
    env, runner = _runner(monkeypatch, steps=8)
    out = capsys.readouterr().out
    assert runner._fused is None and "device LSTM cell unavailable" in out and "512" in out and "up to 256" in out and "torch policy in the rollout" in out


# ---------------------------------------------------------------------------------------------------------------- high_level_game
from tests.game_fixtures import game_registered  # noqa: E402,F401


def test_game_runner_takes_the_separate_launches_behind_a_wide_memory(tmp_path, monkeypatch, game_registered, capsys):
    """``high_level_game`` with ``device_rollout`` + ``wide_memory`` at 288 units: ``lg_lstm_wide_step`` -> ``lg_lstm_wide_actor_act`` ->
    ``lg_game_pre`` -> ``lg_policy_act``, said once; the stored means and values against the float64 module in batch mode; two iterations
    of ``learn``; ``play_game --wide_memory`` on the checkpoint."""
    import os
    from legged_games_gym_amd.rl.recurrent_actor import RecurrentFusedActor
    from legged_games_gym_amd.scripts import play_game as pg
    from tests.test_gpu_game import write_ll_checkpoint as write_ckpt
    from tests.test_gpu_game_recurrent import _check_storage_against_batch_mode as check_game_storage, _game_runner, _stats as game_stats
    ckpt = write_ckpt(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    env, runner = _game_runner(game_registered, tmp_path, monkeypatch, ckpt, units=288, wide_memory=True)
    fused = runner._fused
    assert isinstance(fused, RecurrentFusedActor) and fused.wide and runner._game_rollout and runner._recurrent_rollout
    assert runner.alg.actor_critic.memory_a.rnn.hidden_size == 288 and env.shared_actor_launch(fused) is False
    with torch.inference_mode():
        runner._rollout_steps(game_stats(runner))
        torch.cuda.synchronize()
        check_game_storage(runner, "wide game runner, eager rollout")
    runner.alg.storage.clear()
    runner.learn(2)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(p).all()) for p in runner.alg.actor_critic.parameters())
    said = capsys.readouterr().out
    lines = [l for l in said.splitlines() if "unavailable" in l]
    assert len(lines) == 1 and "wide memory" in lines[0] and "lg_lstm_actor_act + lg_game_pre + lg_policy_act" in lines[0], said
    assert os.path.isfile(os.path.join(runner.log_dir, "model_2.pt"))
    args = pg._args(["--task", "high_level_game", "--num_envs", "16", "--steps", "12", "--headless", "--sim_device", DEV, "--rl_device", DEV,
                     "--policy_class_name", "ActorCriticRecurrent", "--rnn_hidden_size", "288", "--wide_memory", "--load_run", os.path.basename(runner.log_dir)])
    env_p, result, path = pg.play_game(args, steps=args.steps)
    assert result["path"] == "graphed policy step" and result["iteration"] == 2 and result["steps"] == 12 and result["num_envs"] == 16
    assert torch.isfinite(env_p.obs_buf).all()


# ---------------------------------------------------------------------------------------------------------------- DecGamePolicyRunner
from tests.dec_game_fixtures import dec_registered  # noqa: E402,F401
from tests.test_gpu_game import write_ll_checkpoint  # noqa: E402

UNITS_DEC = 288


def _dec_runner(reg, root, monkeypatch, ckpt, n=64, units=UNITS_DEC, **runner_keys):
    import random
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
                     "--policy_class_name", "ActorCriticRecurrent", "--rnn_hidden_size", str(units)])
    apply_policy_args(train_cfg, args)
    torch.manual_seed(4321); np.random.seed(4321); random.seed(4321)
    env, _ = reg.make_env("dec_high_level_game", args)
    torch.manual_seed(1234)
    runner, _ = reg.make_dec_alg_runner(env, "dec_high_level_game", args)
    env.ll_env.episode_length_buf[::2] = int(env.ll_env.max_episode_length) - 3 - (torch.arange(0, n, 2, device=DEV) % 41)
    return env, runner, args


def test_dec_runner_trains_two_wide_recurrent_policies_and_plays(tmp_path, monkeypatch, dec_registered, capsys):
    import os
    from legged_games_gym_amd.rl.recurrent_actor import RecurrentFusedActor
    from legged_games_gym_amd.scripts import play_dec_game as pdg
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    try:
        first_rollouts, runners = [], []
        for run in range(2):
            env, runner, _ = _dec_runner(dec_registered, tmp_path / f"run{run}", monkeypatch, ckpt, wide_memory=True)
            assert runner.recurrent and runner.device_path
            for a in ("pred", "prey"):
                r = runner.runners[a]
                assert isinstance(r._fused, RecurrentFusedActor) and r._fused.wide and r._game_rollout and r._recurrent_rollout
                assert r.alg.actor_critic.memory_a.rnn.hidden_size == UNITS_DEC
            assert env.shared_actor_launch(runner.runners["pred"]._fused, runner.runners["prey"]._fused) is False
            seen = {}
            for a in ("pred", "prey"):                       # every rollout's actions and log-probs, taken where the update begins
                alg = runner.runners[a].alg

                def update(_alg=alg, _update=alg.update, _a=a):
                    seen.setdefault(_a, []).append((_alg.storage.actions.clone(), _alg.storage.actions_log_prob.clone()))
                    return _update()
                monkeypatch.setattr(alg, "update", update)
            torch.manual_seed(99)
            runner.learn(max_num_evolutions=2, num_learning_iterations=1)
            torch.cuda.synchronize()
            assert runner.current_evolution == 2 and set(seen) == {"pred", "prey"}
            assert all(bool(torch.isfinite(p).all()) for a in ("pred", "prey") for p in runner.runners[a].alg.actor_critic.parameters())
            first_rollouts.append(seen["pred"][0])
            runners.append(runner)
        said = capsys.readouterr().out
        lines = [l for l in said.splitlines() if "recurrent actor launch unavailable" in l]
        assert len(lines) == 2 and all("wide memory" in l and "lg_lstm_actor_act x 2 + lg_dec_game_pre + lg_policy_act" in l for l in lines), said      # once per env
        assert [l for l in said.splitlines() if "unavailable" in l] == lines, said      # the device rollout and its graph: not a word
        # determinism: the first rollout of the two runs, step for step
        (act0, lp0), (act1, lp1) = first_rollouts
        assert bool(torch.isfinite(act0).all()) and float(act0.abs().max()) > 0.0
        assert torch.equal(act0, act1) and torch.equal(lp0, lp1)

        runner = runners[-1]
        path = os.path.join(runner.log_dir, "model_2.pt")
        assert os.path.isfile(path)
        args = pdg._args(["--task", "dec_high_level_game", "--num_envs", "32", "--steps", "12", "--outcomes", "--headless", "--sim_device", DEV, "--rl_device", DEV,
                          "--policy_class_name", "ActorCriticRecurrent", "--rnn_hidden_size", str(UNITS_DEC), "--wide_memory",
                          "--load_run", os.path.basename(runner.log_dir)])
        env_p, result, out = pdg.play_outcomes(args, steps=args.steps)
        assert result["iteration"] == 2 and result["steps"] == 12 and result["num_envs"] == 32
        assert torch.isfinite(env_p.obs_buf_prey).all() and torch.isfinite(env_p.obs_buf_pred).all()
    finally:
        _, train_cfg = dec_registered.get_cfgs("dec_high_level_game")              # the registered object is shared: leave it as it was found
        for obj, keys in ((train_cfg.runner, ("device_rollout", "policy_class_name", "wide_memory")), (train_cfg.policy, ("rnn_hidden_size",))):
            for key in keys:
                if key in vars(obj):
                    delattr(obj, key)
