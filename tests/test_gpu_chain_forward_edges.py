"""-m gpu: the chain forward of the wide learner (csrc/lg_policy.h: k_mlp_chain_fwd64<15>, <11> and k_chain_pack, all four layers of up
to two nets in one launch at lg_mlp_wide_set_precision(1)) against float64, element by element, at the edges of its shapes: the
first and last input width of both ranges and each side of every quad boundary of the last k-step, every side of the output write's
lane-group boundaries, one net and two, shared and separate tables of equal and of different ldx, mb around the 32-row half and the
64-row workgroup, 17 workgroups, gathers with repeated rows -- tests/chain_check.py holds the table, tests/test_chain_check.py shows
that the bars used here (the project's own for precision 1: outputs 1e-4 absolute, gradients 3e-4 of each tensor's max + 1e-10) leave
the kernel's arithmetic restated on the CPU at 0.022 .. 0.053 of the output bar and put every planted error 3.9 bars or more out.

Observed on the MI355X, worst fraction of the bar per test: outputs 0.053 (torch float32 0.0035), gradients 0.069 (torch float32
0.0071), one-row probes 0.067, after the in-place step 0.24 (27 000 .. 30 000 bars from the first pass), designed pre-activations
0.063 / 0.038.  Six mutations of the kernel, each built and run once, all fail this file: a zero lo half into layer 1, by2 read from
by's slots, the output predicate one action short, the staging's in1 with ``<`` (only the widths 229, 232, 237, 240, 165, 168, 173, 176
see it), pack_wide_body one column short, act_row from act0 for both halves (gradients and row probes only)."""
import copy

import pytest
import torch

from tests import chain_check as cc
from tests import wide_learner_check as wl

pytestmark = pytest.mark.gpu

IDS = [c.id for c in cc.CASES]
NAN = float("nan")
GUARD_FRONT, GUARD_BACK = 16, 64             # NaN rows before the outputs and behind mb: a whole workgroup of dead rows would land in them


class _Run:
    """One case on the device: deep copies of chain_check's CPU modules and tables, a WideMlpTrainer over them whose output buffers
    are views of larger NaN tensors, and the case's shared float64 reference (CPU)."""

    def __init__(self, cid, nets=None):
        from legged_games_gym_amd.rl.mlp_kernels import WideMlpTrainer
        self.ref = cc.reference(cid)
        inp = self.inp = self.ref.inputs
        self.case, self.mb = inp.case, inp.case.mb
        self.nets = [copy.deepcopy(n).cuda() for n in (nets or inp.nets)]
        first = inp.xs[0].cuda()
        self.xs = [first] + [first if inp.case.shared else x.cuda() for x in inp.xs[1:]]
        self.rows = inp.rows.cuda() if inp.rows is not None else None
        self.tr = tr = WideMlpTrainer(self.nets, self.xs, self.mb)
        assert tr.supported and not tr.has_fused_minibatch
        self.guarded = [torch.full((GUARD_FRONT + self.mb + GUARD_BACK, o), NAN, device="cuda") for _, o in inp.case.nets]
        tr.outputs = [g[GUARD_FRONT:GUARD_FRONT + self.mb] for g in self.guarded]
        tr.refresh()
        self.labels = wl.param_labels(self.nets)

    def forward(self):
        return self.tr.forward(self.rows)

    def backward(self, d_out):
        """.grad of every parameter for ``d_out``; the tensors are NaN before the launch (the kernels overwrite every element)."""
        for net in self.nets:
            for p in net.parameters():
                p.grad.fill_(NAN)
        for buf, d in zip(self.tr.grad_outputs, d_out):
            buf.copy_(d)
        self.tr.backward(self.rows)
        return [p.grad for n in self.nets for p in n.parameters()]

    def guards_untouched(self):
        for n, g in enumerate(self.guarded):
            front, back = g[:GUARD_FRONT], g[GUARD_FRONT + self.mb:]
            assert bool(torch.isnan(front).all()), f"net {n}: {int((~torch.isnan(front)).sum())} elements written before the outputs"
            assert bool(torch.isnan(back).all()), f"net {n}: {int((~torch.isnan(back)).sum())} elements written behind row mb - 1"


@pytest.fixture
def precision_1():
    from legged_games_gym_amd import capi
    lib = capi.load_library()
    old = lib.lg_mlp_wide_set_precision(cc.PRECISION)
    try:
        yield lib
    finally:
        lib.lg_mlp_wide_set_precision(old)


def _one_row(run, r, d_row=None, seed=0):
    """d_out that is zero except in row ``r`` (randn there unless given), and that row per net; CPU tensors, copied in by backward()."""
    g = torch.Generator().manual_seed(1000 * seed + r)
    d_row = d_row or [torch.randn(o, generator=g) for _, o in run.case.nets]
    d_out = [torch.zeros(run.mb, o) for _, o in run.case.nets]
    for d, v in zip(d_out, d_row):
        d[r] = v
    return d_out, d_row


@pytest.mark.parametrize("cid", IDS)
def test_outputs_match_float64_element_by_element_with_guards(cid, precision_1):
    """Every output element against the float64 module on the gathered rows, at the project's bar for precision 1 (1e-4 absolute).
    The workspace is NaN before the launch: whatever the chain reads of it -- the padded input rows, the packed operand streams, the
    padded biases -- was written by k_wide_prep / k_chain_pack in the same call, or the outputs are NaN.  The output buffers sit
    inside larger NaN tensors of the test's own: a row written before row 0 or behind row mb - 1 shows there."""
    run = _Run(cid)
    run.tr.workspace.fill_(NAN)
    outs = run.forward()
    torch.cuda.synchronize()
    print(f"[observed] chain {cid} {list(run.case.nets)} mb {run.mb}: outputs {wl.max_error([o.cpu() for o in outs], run.ref.want_out, False) / cc.OUT_BAR:.4f} of the bar "
          f"(torch f32 {run.ref.f32_out_err / cc.OUT_BAR:.4f})")
    wl.compare_all([f"net{n}.output" for n in range(len(outs))], outs, run.ref.want_out, abs_tol=cc.OUT_BAR)
    run.guards_untouched()


@pytest.mark.parametrize("cid", IDS)
def test_parameter_gradients_match_float64(cid, precision_1):
    """forward, then backward for d_out = randn / mb: every parameter gradient against float64 autograd at 3e-4 of the tensor's max
    + 1e-10 -- the check of test_wide_mlp_kernels_match_autograd at the table's shapes; the backward reads the activations the chain
    saved (act[0..2]) and the padded input rows it shared with k_wide_prep."""
    run = _Run(cid)
    run.forward()
    got = run.backward(run.ref.d_out)
    torch.cuda.synchronize()
    print(f"[observed] chain {cid} mb {run.mb}: gradients {wl.max_error([g.cpu() for g in got], run.ref.want_grads, True) / cc.GRAD_BAR:.4f} of the bar "
          f"(torch f32 {run.ref.f32_grad_err / cc.GRAD_BAR:.4f})")
    wl.compare_all(run.labels, got, run.ref.want_grads, rel=cc.GRAD_BAR, abs_tol=cc.GRAD_ABS)
    run.guards_untouched()


@pytest.mark.parametrize("cid", cc.ROW_PROBE_CASES)
def test_saved_activations_row_by_row(cid, precision_1):
    """One forward pass, then one backward pass per probed row r with d_out zero except in row r: dW_3 = d_out[r]^T . act_2[r] and the
    lower layers likewise, so every gradient's maximum is that ROW's own scale and a wrong saved-activation row at a half or workgroup
    boundary (rows 31 | 32, 63 | 64, mb - 1) cannot hide behind the other rows of the mini-batch.  float64 autograd of the same
    one-row d_out, the gradient bar."""
    run = _Run(cid)
    run.forward()
    probes = sorted({min(r, run.mb - 1) for r in cc.ROW_PROBES + (run.mb - 1,)})
    worst = 0.0
    for r in probes:
        d_out, d_row = _one_row(run, r)
        got = run.backward(d_out)
        want = cc.one_row_grads(run.ref, r, d_row)
        worst = max(worst, wl.compare_all([f"row {r}: {l}" for l in run.labels], got, want, rel=cc.GRAD_BAR, abs_tol=cc.GRAD_ABS))
    print(f"[observed] chain {cid} mb {run.mb}: rows {probes} probed one at a time, gradients {worst / cc.GRAD_BAR:.4f} of the bar")


@pytest.mark.parametrize("k", [15, 11])
def test_the_forward_follows_an_in_place_parameter_step(k, precision_1):
    """k_chain_pack re-packs the operand streams on every call: after an in-place change of all eight tensors of each net (addresses
    unchanged, no refresh()) the next forward pass computes the NEW parameters' outputs -- and those are far from the old ones."""
    run = _Run(cc.BASE[k])
    first = [o.clone() for o in run.forward()]
    g = torch.Generator(device="cuda").manual_seed(3)
    with torch.no_grad():
        for net in run.nets:
            assert len(list(net.parameters())) == 8
            for p in net.parameters():
                p.add_(0.05 * torch.randn(p.shape, device="cuda", generator=g))
    refs = [wl.float64_copy(n).cpu() for n in run.nets]
    with torch.no_grad():
        want = [r(x.double()) for r, x in zip(refs, run.ref.xb)]
    second = run.forward()
    moved = cc.bars_out([s.cpu() for s in second], [f.cpu() for f in first])
    print(f"[observed] chain {cc.BASE[k]}: after the step {wl.max_error([s.cpu() for s in second], want, False) / cc.OUT_BAR:.4f} of the bar, {moved:.0f} bars from the first pass")
    wl.compare_all([f"net{n}.output" for n in range(len(second))], second, want, abs_tol=cc.OUT_BAR)
    assert moved >= 100.0
    run.guards_untouched()


DESIGNED_BIASES = (0.0, -1e-6, -30.0, -100.0, -1e4, 8.0)


@pytest.mark.parametrize("k", [15, 11])
def test_designed_pre_activations(k, precision_1):
    """In each hidden layer six units get a zero weight row and a bias from {0, -1e-6, -30, -100, -1e4, 8}: their pre-activation is
    exactly the bias in every row.  Outputs and gradients stay finite and inside the bars (float64: exp(-1e4) - 1 = -1, no overflow
    on the way); and, read off through a one-row probe (dW_{l+1}[:, u] = delta_{l+1}[r] * act_l[r, u], db_{l+1} = delta_{l+1}[r]):
    the unit at 0 has the activation exactly 0 -- its column of dW_{l+1} is exactly zero -- and the units at -100 and -1e4 exactly
    -1: on the output layer (plain float32 FMAs in k_wide_out_bwd) their columns are exactly -db_3, on the hidden layers (split-bf16
    GEMM: delta enters as hi + lo) exactly -(hi + lo)(db)."""
    cid = cc.BASE[k]
    nets = [copy.deepcopy(n) for n in cc.inputs(cid).nets]
    units = {0: (3, 200, 77, 500, 31, 32), 1: (0, 255, 100, 64, 33, 129), 2: (127, 0, 63, 64, 31, 96)}      # per hidden layer, both sides of tile edges
    with torch.no_grad():
        for net in nets:
            layers = [m for m in net if isinstance(m, torch.nn.Linear)]
            for l, us in units.items():
                for u, b in zip(us, DESIGNED_BIASES):
                    layers[l].weight[u].zero_()
                    layers[l].bias[u] = b
    run = _Run(cid, nets=nets)
    refs = [wl.float64_copy(n) for n in nets]
    want_out = [r(x.double()) for r, x in zip(refs, run.ref.xb)]
    torch.autograd.backward(want_out, [d.double() for d in run.ref.d_out])
    want = [p.grad for r in refs for p in r.parameters()]
    outs = run.forward()
    o_fig = wl.compare_all([f"net{n}.output" for n in range(len(outs))], outs, [w.detach() for w in want_out], abs_tol=cc.OUT_BAR)
    g_fig = wl.compare_all(run.labels, run.backward(run.ref.d_out), want, rel=cc.GRAD_BAR, abs_tol=cc.GRAD_ABS)
    print(f"[observed] chain {cid} designed pre-activations: outputs {o_fig / cc.OUT_BAR:.4f}, gradients {g_fig / cc.GRAD_BAR:.4f} of the bars")
    for r in (0, 32, run.mb - 1):
        d_out, _ = _one_row(run, r, seed=1)
        run.backward(d_out)
        for n, net in enumerate(run.nets):
            layers = [m for m in net if isinstance(m, torch.nn.Linear)]
            for l, us in units.items():
                dw, db = layers[l + 1].weight.grad.cpu(), layers[l + 1].bias.grad.cpu()
                assert float(db.abs().max()) > 0.0
                hi, lo = cc.split(db)
                minus_one = -db if l == 2 else -(hi + lo)
                assert not dw[:, us[0]].any(), f"net {n} row {r} layer {l}: the unit at bias 0 has a non-zero activation"
                for u in (us[3], us[4]):
                    assert torch.equal(dw[:, u], minus_one), f"net {n} row {r} layer {l} unit {u}: activation not exactly -1 ({float((dw[:, u] - minus_one).abs().max()):.3e})"
                assert float(dw[:, us[5]].abs().max()) > 0.0 and float(dw[:, us[1]].abs().max()) > 0.0
    run.guards_untouched()


def test_bit_identical_from_run_to_run(precision_1):
    """Forward + backward twice on the 1025-row case: the same bits in every output and gradient (fixed reduction order, no atomics)."""
    run = _Run(cc.REPEAT)
    first = [o.clone() for o in run.forward()] + [g.clone() for g in run.backward(run.ref.d_out)]
    for o in run.tr.outputs:
        o.fill_(NAN)
    second = list(run.forward()) + run.backward(run.ref.d_out)
    assert len(first) == len(second) == len(run.nets) + len(run.labels)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    assert all(bool(torch.isfinite(a).all()) for a in first)


def test_every_case_takes_the_chain_rule_restated():
    """Every case satisfies the host rule of lg_mlp_wide_forward for the chain, as wide_learner_check restates it (the generic-path
    test asserts the opposite of its cases).  The library offers no way to ask which kernel ran, and none is added for this: that the
    rule restated is the rule compiled is checked against the source text by tests/test_chain_check.py."""
    for case in cc.CASES:
        assert not wl.takes_generic_forward(cc.spec(case)), case.id
    cc.assert_the_host_rule()
