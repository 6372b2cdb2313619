"""Shared pieces of tests/test_gpu_lstm_sequence.py, tests/test_gpu_lstm_sequence_edges.py (GPU) and tests/test_lstm_seq_check.py (CPU):
the input recipe of the LSTM sequence tests, the case table that takes ``k_lstm_seq_pack`` / ``k_lstm_seq_fwd`` / ``k_lstm_seq_bwd``
(csrc/lg_lstm_seq.hip) to their shape edges, the launch arithmetic of those kernels restated, an explicit float64 restatement of the
forward and of back-propagation through time, the same two functions in float32 as the control, planted errors, and the bars.  CPU torch
only; nothing here touches the device library, so the table's reach claims and the bars' controls are tested without a GPU.

Edges: a workgroup has ``H / 32`` waves (1 .. 8); the forward's gate GEMM runs ``ksteps = (I + H + 1) / 2`` k-steps as ``ksteps / 4``
prefetched groups and a tail of ``ksteps % 4``, with a zero pad row at odd ``K = I + H``; ``x_t`` is staged by ``2 H`` threads walking
``(k += x_dk, row += x_drow)`` over ``32 I`` elements; a workgroup owns 32 trajectory rows, the last one ``B % 32`` of them."""
import functools
import types
from collections import namedtuple

import torch
import torch.nn as nn

from tests.recurrent_ref import saturating_bias
from tests.wide_learner_check import GRAD_ABS, GRAD_TOL

TOL = 2e-5                               # TOL of tests/test_gpu_recurrent.py: gates absolute, h and c of max(1, max |want|)
GRAD_REL = GRAD_TOL[0]                   # 1e-4 of max |want| (+ GRAD_ABS): dG and the weight gradients
PARAMS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
BLOCK_ROWS = 32                          # LG_LSTM_SEQ_BLOCK_ROWS
UPDATE_T = 24                            # num_steps_per_env of the registered tasks: the padded trajectories' T in PPO.update
ROUGH_OBS, FLAT_OBS, MAX_IN = 235, 48, 256
# float64 against float64: 2.2e-16 per operation, a few thousand of them on the way to any element (T B <= 1585 terms in a weight
# gradient, <= 48 steps of recurrence); seven orders below the tightest bar
RESTATEMENT_TOL = 1e-12

# (T, B, I, H) of tests/test_gpu_lstm_sequence.py: one of everything | odd K = 51 and one row past a block | 2 waves | the update's T |
# an exact block and 8 waves | the rough task's K = 491 (odd) | the largest LDS blocks, three workgroups
OLD_SHAPES = ((1, 1, 1, 32), (2, 33, 19, 32), (3, 5, 17, 64), (24, 37, 48, 64), (24, 32, 48, 256), (5, 64, 235, 256), (24, 96, 256, 256))

Case = namedtuple("Case", "shape why")
# the smallest shapes at which each mechanism exists; none is a workload size
CASES = (
    Case((24, 33, 13, 96), "3 waves; odd K, tail of 3; one row past a block; ragged staging (416 elements, 192 threads)"),
    Case((24, 31, 48, 128), "4 waves; the flat task's 48 observations; one row short of a block"),
    Case((24, 65, 17, 160), "5 waves; odd K, tail of 1; three workgroups, the last with one live row"),
    Case((6, 33, 6, 192), "6 waves; tail of 3 without the pad row"),
    Case((24, 32, 39, 224), "7 waves; pad row with no tail; exact block"),
    Case((3, 4, 2, 224), "7 waves; even K, tail of 1; rows of one lane half only"),
    Case((3, 37, 4, 128), "4 waves; tail of 2, even K"),
    Case((3, 33, 235, 32), "1 wave; I > 2H: x_drow == 0"),
    Case((3, 5, 64, 32), "1 wave; I == 2H: x_dk == 0, x_drow == 1"),
    Case((2, 64, 256, 64), "2 waves; largest I on 128 threads"),
    Case((4, 32, 32, 64), "2 waves; I divides 2H and every thread stages eight elements"),
    Case((2, 33, 1, 256), "8 waves; one input, fewer staged elements than threads"),
    Case((48, 33, 48, 128), "4 waves; twice the update's T: drift through time"),
)
SHAPES = tuple(c.shape for c in CASES)
TIMES_THREE = ((24, 33, 13, 96), (24, 65, 17, 160))      # run a second time with every parameter x 3: gates pushed towards saturation
FOLLOW = (24, 31, 48, 128)               # the forward follows the parameters
REPEAT = (24, 65, 17, 160)               # bit-identical repeats


def case(shape):
    return CASES[SHAPES.index(tuple(shape))]


def launch(shape):
    """What lg_lstm_seq_create / k_lstm_seq_fwd derive from a shape (csrc/lg_lstm_seq.hip), restated."""
    T, B, I, H = shape
    K, nthreads = I + H, 2 * H
    ksteps = (K + 1) // 2
    return types.SimpleNamespace(
        waves=H // 32, K=K, odd=bool(K & 1), ksteps=ksteps, groups=ksteps // 4, tail=ksteps % 4, nthreads=nthreads,
        n_x=32 * I, x_drow=nthreads // I, x_dk=nthreads % I, blocks=-(-B // BLOCK_ROWS), last_rows=B - BLOCK_ROWS * ((B - 1) // BLOCK_ROWS),
        fwd_lds=2 * ksteps * 33 * 4, bwd_lds=4 * H * 33 * 4)


def staging(shape):
    """The regime of the x staging walk: 'one' (a single input) | 'divides' (x_dk == 0, I < 2H) | 'equal' (I == 2H) | 'above' (I > 2H,
    x_drow == 0) | 'below' (I < 2H, not a divisor: both x_dk and x_drow non-zero)."""
    I, L = shape[2], launch(shape)
    if I == 1:
        return "one"
    if I == L.nthreads:
        return "equal"
    if I > L.nthreads:
        return "above"
    return "divides" if L.x_dk == 0 else "below"


def make_inputs(shape, scale=1.0, saturate=False):
    """(rnn, x [T, B, I], h0, c0 [B, H], dh [T, B, H], lengths [B]) in float32 on the CPU: trajectory lengths in 1 .. T (trajectory 0
    full), ``x`` and ``dh`` zero beyond each length, ``h0`` / ``c0`` non-zero; every parameter of torch's default ``nn.LSTM`` times
    ``scale``; ``saturate`` adds ``recurrent_ref.saturating_bias`` to ``bias_ih_l0``."""
    T, B, I, H = shape
    torch.manual_seed(1000 * T + 10 * B + I + H)
    rnn = nn.LSTM(I, H)
    with torch.no_grad():
        for p in rnn.parameters():
            p.mul_(scale)
        if saturate:
            rnn.bias_ih_l0.add_(torch.from_numpy(saturating_bias(H)).float())
    gen = torch.Generator().manual_seed(7 * T + B)
    lengths = torch.randint(1, T + 1, (B,), generator=gen)
    lengths[0] = T
    live = (torch.arange(T).unsqueeze(1) < lengths.unsqueeze(0)).float().unsqueeze(-1)          # [T, B, 1]
    x = (torch.rand(T, B, I, generator=gen) * 6.0 - 3.0) * live
    dh = torch.randn(T, B, H, generator=gen) * live
    h0, c0 = torch.rand(B, H, generator=gen) * 2 - 1, torch.rand(B, H, generator=gen) * 2 - 1
    return rnn, x, h0, c0, dh, lengths


def params_of(rnn):
    return tuple(getattr(rnn, n).detach().cpu() for n in PARAMS)


# ---------------------------------------------------------------------------------------------------------------- the restatement
FORWARD_FAULTS = ("x_column_dropped", "h_column_dropped", "x_rows_exchanged")
BACKWARD_FAULTS = ("c0_taken_as_zero", "dc_carry_dropped", "k_row_dropped", "dh_rec_rows_exchanged")


def _exchanged(v, dim):
    """Rows 0 (a full trajectory) and B - 1 (the last row of the last block) of ``v`` along ``dim`` exchanged."""
    idx = list(range(v.shape[dim]))
    idx[0], idx[-1] = idx[-1], idx[0]
    return v.index_select(dim, torch.tensor(idx))


def forward(params, x, h0, c0, dtype=torch.float64, fault=None):
    """The LSTM written out: (gates [T, B, 4H] = sigma, sigma, tanh, sigma of the i, f, g, o blocks of b_ih + b_hh + W_ih x_t + W_hh h_{t-1},
    c [T, B, H] = f c_{t-1} + i g, h [T, B, H] = o tanh(c)) in ``dtype``.  ``fault``: one of FORWARD_FAULTS."""
    assert fault is None or fault in FORWARD_FAULTS
    w_ih, w_hh, b_ih, b_hh = (p.detach().to(dtype) for p in params)
    x, h, c = x.to(dtype), h0.to(dtype), c0.to(dtype)
    H = w_hh.shape[1]
    if fault == "x_column_dropped":
        w_ih = w_ih.clone()
        w_ih[:, -1] = 0.0
    if fault == "h_column_dropped":
        w_hh = w_hh.clone()
        w_hh[:, -1] = 0.0
    if fault == "x_rows_exchanged":
        x = _exchanged(x, 1)
    gates, cs, hs = [], [], []
    for t in range(x.shape[0]):
        a = (b_ih + b_hh) + x[t] @ w_ih.t() + h @ w_hh.t()
        i, f, g, o = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H]), torch.tanh(a[:, 2 * H:3 * H]), torch.sigmoid(a[:, 3 * H:])
        c = f * c + i * g
        h = o * torch.tanh(c)
        gates.append(torch.cat((i, f, g, o), 1))
        cs.append(c)
        hs.append(h)
    return torch.stack(gates), torch.stack(cs), torch.stack(hs)


def backward(params, gates, c, c0, dh, dtype=torch.float64, fault=None):
    """Back-propagation through time by hand, from the forward's ``gates`` and ``c``: dG [T, B, 4H], the gradient of sum(h * dh) with
    respect to the four pre-activation blocks.  ``fault``: one of BACKWARD_FAULTS."""
    assert fault is None or fault in BACKWARD_FAULTS
    w_hh = params[1].detach().to(dtype)
    gates, c, c0, dh = gates.to(dtype), c.to(dtype), c0.to(dtype), dh.to(dtype)
    T, B, H = c.shape
    dh_rec, dc_rec = torch.zeros(B, H, dtype=dtype), torch.zeros(B, H, dtype=dtype)
    out = [None] * T
    for t in range(T - 1, -1, -1):
        i, f, g, o = gates[t, :, :H], gates[t, :, H:2 * H], gates[t, :, 2 * H:3 * H], gates[t, :, 3 * H:]
        c_prev = c[t - 1] if t > 0 else (torch.zeros_like(c0) if fault == "c0_taken_as_zero" else c0)
        d_h = dh[t] + dh_rec
        tc = torch.tanh(c[t])
        d_c = dc_rec + d_h * o * (1.0 - tc * tc)
        da = torch.cat((d_c * g * (i * (1.0 - i)), d_c * c_prev * (f * (1.0 - f)), d_c * i * (1.0 - g * g), d_h * tc * (o * (1.0 - o))), 1)
        out[t] = da
        dc_rec = torch.zeros_like(d_c) if fault == "dc_carry_dropped" else d_c * f
        dh_rec = da[:, :-1] @ w_hh[:-1] if fault == "k_row_dropped" else da @ w_hh
        if fault == "dh_rec_rows_exchanged":
            dh_rec = _exchanged(dh_rec, 0)
    return torch.stack(out)


def weight_grads(dG, x, h, h0):
    """(dW_ih = dG^T x, dW_hh = dG^T h_prev, db = column sums of dG) over all T B rows, in dG's type."""
    T, B, H4 = dG.shape
    d = dG.reshape(T * B, H4)
    h_prev = torch.cat((h0.to(dG.dtype).unsqueeze(0), h.to(dG.dtype)[:-1]), 0).reshape(T * B, -1)
    return d.t() @ x.to(dG.dtype).reshape(T * B, -1), d.t() @ h_prev, d.sum(0)


def restate(params, x, h0, c0, dh, dtype=torch.float64, forward_fault=None, backward_fault=None):
    """Forward, BPTT and the weight gradients of one set of parameters: gates, c, h, dG, dw_ih, dw_hh, db."""
    gates, c, h = forward(params, x, h0, c0, dtype, forward_fault)
    dG = backward(params, gates, c, c0, dh, dtype, backward_fault)
    dw_ih, dw_hh, db = weight_grads(dG, x, h, h0)
    return types.SimpleNamespace(gates=gates, c=c, h=h, dG=dG, dw_ih=dw_ih, dw_hh=dw_hh, db=db)


def lstm_autograd64(params, x, h0, c0, dh):
    """float64 ``nn.LSTM`` with autograd on the same inputs: (h [T, B, H], dW_ih, dW_hh, db_ih, db_hh)."""
    net = nn.LSTM(x.shape[2], h0.shape[1]).double()
    with torch.no_grad():
        for n, p in zip(PARAMS, params):
            getattr(net, n).copy_(p.double())
    out, _ = net(x.double(), (h0.double().unsqueeze(0), c0.double().unsqueeze(0)))
    (out * dh.double()).sum().backward()
    return (out.detach(),) + tuple(getattr(net, n).grad for n in PARAMS)


def assert_restatement_agrees(label, want, params, x, h0, c0, dh):
    h, dw_ih, dw_hh, db_ih, db_hh = lstm_autograd64(params, x, h0, c0, dh)
    figs = {}
    for name, got, ref in (("h", want.h, h), ("dw_ih", want.dw_ih, dw_ih), ("dw_hh", want.dw_hh, dw_hh), ("db", want.db, db_ih), ("db", want.db, db_hh)):
        figs[name] = float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)
        assert figs[name] < RESTATEMENT_TOL, f"{label}: the restatement's {name} is {figs[name]:.3e} of its maximum from float64 nn.LSTM autograd"
    return figs


# ---------------------------------------------------------------------------------------------------------------- the bars
FORWARD_QUANTITIES, BACKWARD_QUANTITIES = ("gates", "h", "c"), ("dG", "dw_ih", "dw_hh", "db")


def bar(name, want):
    """The bound on max |got - want| of one quantity."""
    w = getattr(want, name)
    if name == "gates":
        return TOL
    if name in ("h", "c"):
        return TOL * max(1.0, float(w.abs().max()))
    return GRAD_REL * float(w.abs().max()) + GRAD_ABS


def fractions(got, want, names):
    """max |got - want| of each named quantity as a fraction of its bar (float64, on the CPU)."""
    return {n: float((getattr(got, n).detach().double().cpu() - getattr(want, n)).abs().max()) / bar(n, want) for n in names}


@functools.lru_cache(maxsize=None)
def reference(shape, scale=1.0):
    """Inputs, the float64 restatement and the float32 control of a case (all on the CPU; computed once, never modified).  The restatement is asserted against float64 ``nn.LSTM`` autograd here, once."""
    rnn, x, h0, c0, dh, lengths = make_inputs(tuple(shape), scale)
    params = params_of(rnn)
    want = restate(params, x, h0, c0, dh)
    agreement = assert_restatement_agrees(f"{shape} x {scale:g}", want, params, x, h0, c0, dh)
    ctrl = restate(params, x, h0, c0, dh, torch.float32)
    live = torch.arange(shape[0]).unsqueeze(1) < lengths.unsqueeze(0)                             # [T, B]
    return types.SimpleNamespace(shape=tuple(shape), scale=scale, rnn=rnn, params=params, x=x, h0=h0, c0=c0, dh=dh, lengths=lengths, live=live,
                                 want=want, ctrl=ctrl, agreement=agreement)


def as_case(ref):
    """The dict tests/test_gpu_lstm_sequence.py's helpers take."""
    return dict(shape=ref.shape, rnn=ref.rnn, x=ref.x, h0=ref.h0, c0=ref.c0, dh=ref.dh, lengths=ref.lengths, want_h=ref.want.h, want_c=ref.want.c,
                want_grads=[ref.want.dw_ih, ref.want.dw_hh, ref.want.db, ref.want.db])
