"""-m gpu: ``k_lstm_seq_pack`` / ``k_lstm_seq_fwd`` / ``k_lstm_seq_bwd`` (csrc/lg_lstm_seq.hip) at their shape edges, element by element.

The cases, their inputs, the explicit float64 restatement (forward with the gates, back-propagation through time by hand down to ``dG``)
and the bars are those of tests/lstm_seq_check.py; tests/test_lstm_seq_check.py shows on the CPU that the table reaches 3 .. 7 waves, every
(K parity, ksteps % 4) pair and every regime of the x staging walk, that float32 arithmetic is within a quarter of every bar and that a
misplaced column, row or k-step is at least ten bars out.  Bars: gates absolute ``TOL = 2e-5``; ``h`` and ``c`` at
``TOL * max(1, max |want|)``; ``dG`` and the weight gradients through ``wide_learner_check.compare`` with ``rel = 1e-4`` of ``max |want|``
plus ``GRAD_ABS``.

a. forward, raw entry point: ``h_out``, ``c`` and the four gate blocks of the workspace against float64; NaN guards; ``ws == NULL``;
b. backward, raw entry point: ``dG`` element by element, exactly 0 at every padded (t, row); the ``c`` block untouched; NaN guards;
c. the four parameter gradients through ``DeviceLstmSequence``; d. the rollout cell stepped T times;
e. a parameter change between two forwards of one ``DeviceLstmSequence`` and of one handle is followed (the pack runs every time);
f. weights x 3 on two cases; g. bit-identical repeats on three workgroups of 5 waves.

Measured on one MI355X, worst over the table, as fractions of the bars (every test prints its own with an ``[observed]`` prefix; in
brackets the float32 control of tests/test_lstm_seq_check.py on the CPU):
    gates 0.080 (block g, I = 235; i, f, o at most 0.038) [0.095];  h 0.067 (I = 235) [0.070];  c 0.034 [0.032];  dG 0.0078 [0.0059];
    dW_ih 0.011 [0.006];  dW_hh 0.013 [0.008];  db 0.0057 [0.0043];  with weights x 3: gates 0.062 [0.080], h 0.029, dG 0.0075.
dG was exactly 0 at every padded (t, row) of every case.  Against the stepped rollout cell: at most 2.7e-7 (bar 2e-5), bit-equal in no
case.  After the optimiser-like parameter change the second output is 44000 (module) and 48000 (one handle) bars from the first.  No case
faulted and no kernel was changed.
"""
import copy
import ctypes as C

import pytest
import torch

from tests import lstm_seq_check as lc
from tests import test_gpu_lstm_sequence as S
from tests.wide_learner_check import GRAD_ABS, compare

pytestmark = pytest.mark.gpu
DEV = S.DEV
PARAMS = lc.PARAMS


def _raw(ref, rnn=None):
    """Forward with a workspace, then backward, through the raw entry points with NaN guards behind every buffer, inputs included."""
    T, B, I, H = ref.shape
    case = lc.as_case(ref)
    if rnn is not None:
        case["rnn"] = rnn
    run = S._forward(case)
    lib = run["lib"]
    ws_fwd = run["ws"].clone()
    padded = {}
    for name, src in (("dh", ref.dh), ("w_hh", run["rnn"].weight_hh_l0.detach()), ("c0", ref.c0)):
        whole, view = S._guarded(src.numel())
        view.copy_(src.reshape(-1))
        padded[name] = (whole, view)
    rc = lib.lg_lstm_seq_backward(run["handle"], padded["w_hh"][1].data_ptr(), padded["dh"][1].data_ptr(), padded["c0"][1].data_ptr(),
                                  run["ws"].data_ptr(), T, B, S._stream())
    assert rc == 0, lib.lg_lstm_seq_last_error()
    torch.cuda.synchronize()
    guards = [("h_out", run["h_whole"][T * B * H:]), ("ws", run["ws_whole"][5 * T * B * H:])] + [(n, w[v.numel():]) for n, (w, v) in padded.items()]
    return run, ws_fwd, guards


def _got(ref, h_out, ws_fwd=None, ws_bwd=None):
    T, B, I, H = ref.shape
    n = 4 * T * B * H
    got = dict(h=h_out.view(T, B, H))
    if ws_fwd is not None:
        got.update(gates=ws_fwd[:n].view(T, B, 4 * H), c=ws_fwd[n:].view(T, B, H))
    if ws_bwd is not None:
        got.update(dG=ws_bwd[:n].view(T, B, 4 * H))
    return got


def _check(tag, ref, want, got):
    """Every quantity of ``got`` finite and inside its bar; the gates block by block.  Prints the fractions of the bars."""
    T, B, I, H = ref.shape
    figs = {}
    for name, g in got.items():
        assert bool(torch.isfinite(g).all()), f"{tag} {ref.shape}: {name} has non-finite elements (not written?)"
        w = getattr(want, name)
        if name in ("dG", "dw_ih", "dw_hh", "db"):
            compare(f"{tag} {ref.shape} {name}", g, w, rel=lc.GRAD_REL, abs_tol=GRAD_ABS)
            figs[name] = float((g.double().cpu() - w).abs().max()) / lc.bar(name, want)
        elif name == "gates":
            err = (g.double().cpu() - w).abs()
            blocks = [float(err[..., k * H:(k + 1) * H].max()) for k in range(4)]
            figs.update({f"gate {n}": e / lc.TOL for n, e in zip("ifgo", blocks)})
        else:
            figs[name] = float((g.double().cpu() - w).abs().max()) / lc.bar(name, want)
    print(f"[observed] {tag} {ref.shape} x {ref.scale:g}: " + ", ".join(f"{k} {v:.4f}" for k, v in figs.items()) + " of the bars")
    for name, fig in figs.items():
        assert fig < 1.0, f"{tag} {ref.shape}: {name} is {fig:.3f} bars from float64"
    return figs


def _check_forward(tag, ref):
    case = lc.as_case(ref)
    run = S._forward(case)
    T, B, I, H = ref.shape
    _check(tag, ref, ref.want, _got(ref, run["h_out"], run["ws"]))
    assert torch.isnan(run["h_whole"][T * B * H:]).all(), "the guard behind h_out was written"
    assert torch.isnan(run["ws_whole"][5 * T * B * H:]).all(), "the guard behind ws was written"
    bare = S._forward(case, with_ws=False)
    assert torch.equal(bare["h_out"], run["h_out"]), "ws == NULL changes h_out"
    assert torch.isnan(bare["h_whole"][T * B * H:]).all()
    for r in (run, bare):
        assert r["lib"].lg_lstm_seq_destroy(r["handle"]) == 0


def _check_backward(tag, ref):
    T, B, I, H = ref.shape
    run, ws_fwd, guards = _raw(ref)
    got = _got(ref, run["h_out"], None, run["ws"])
    _check(tag, ref, ref.want, dict(dG=got["dG"]))
    dead = ~ref.live
    assert int(dead.sum()) == T * B - int(ref.lengths.sum())
    stray = got["dG"].cpu()[dead]
    assert not stray.any(), f"dG is not exactly 0 at {int(stray.any(-1).sum())} of {int(dead.sum())} padded (t, row)"
    assert torch.equal(run["ws"][4 * T * B * H:], ws_fwd[4 * T * B * H:]), "the backward wrote into the c block of the workspace"
    for name, g in guards:
        assert g.numel() > 0 and torch.isnan(g).all(), f"the guard behind {name} was written"
    assert run["lib"].lg_lstm_seq_destroy(run["handle"]) == 0


def _check_module(tag, ref):
    """``S._check_backward``: out and the four gradients at the sequence tests' bars, db_ih bit-equal to db_hh; the figures per tensor."""
    out, grads = S._check_backward(lc.as_case(ref), tag)
    _check(tag, ref, ref.want, dict(h=out, dw_ih=grads[0], dw_hh=grads[1], db=grads[2]))


# ---------------------------------------------------------------------------------------------------------------- a. - d. over the table
@pytest.mark.parametrize("shape", lc.SHAPES)
def test_forward_gates_c_and_h_match_float64_element_by_element(shape):
    _check_forward("forward", lc.reference(shape))


@pytest.mark.parametrize("shape", lc.SHAPES)
def test_backward_dG_matches_float64_element_by_element(shape):
    _check_backward("backward", lc.reference(shape))


@pytest.mark.parametrize("shape", lc.SHAPES)
def test_parameter_gradients_through_the_module_match_float64(shape):
    _check_module("module", lc.reference(shape))


@pytest.mark.parametrize("shape", lc.SHAPES)
def test_forward_matches_the_rollout_cell_stepped_through_time(shape):
    S._check_against_the_stepped_cell(lc.as_case(lc.reference(shape)))


# ---------------------------------------------------------------------------------------------------------------- e. the repack
def _changed(rnn, seed):
    """An optimiser-like step on all four tensors, in place; the new parameters as read back from the device and their float64 results."""
    gen = torch.Generator().manual_seed(seed)
    ptrs = [getattr(rnn, n).data_ptr() for n in PARAMS]
    with torch.no_grad():
        for n in PARAMS:
            p = getattr(rnn, n)
            p.add_((0.05 * torch.randn(p.shape, generator=gen)).to(DEV))
    assert ptrs == [getattr(rnn, n).data_ptr() for n in PARAMS]
    return lc.params_of(rnn)


def _restated(ref, params, label):
    want = lc.restate(params, ref.x, ref.h0, ref.c0, ref.dh)
    lc.assert_restatement_agrees(label, want, params, ref.x, ref.h0, ref.c0, ref.dh)
    return want


def _moved(tag, first, second, want):
    """The second output in bars of ``h`` from the first: the check cannot pass on stale weights."""
    bars = float((second.double() - first.double()).abs().max()) / lc.bar("h", want)
    print(f"[observed] {tag}: the second output is {bars:.0f} bars from the first")
    assert bars > 100.0
    return bars


def test_the_forward_follows_the_parameters_through_the_module():
    from legged_games_gym_amd.rl.lstm_sequence import DeviceLstmSequence
    ref = lc.reference(lc.FOLLOW)
    rnn = copy.deepcopy(ref.rnn).to(DEV)
    seq = DeviceLstmSequence(rnn, DEV)
    x, state, dh = ref.x.to(DEV), (ref.h0.to(DEV).unsqueeze(0), ref.c0.to(DEV).unsqueeze(0)), ref.dh.to(DEV)

    def both_ways():
        rnn.zero_grad(set_to_none=True)
        out = seq(x, state)
        out.backward(dh)
        torch.cuda.synchronize()
        grads = [getattr(rnn, n).grad.clone() for n in PARAMS]
        assert torch.equal(grads[2], grads[3]), "db_ih != db_hh"
        return out.detach().clone(), dict(dw_ih=grads[0], dw_hh=grads[1], db=grads[2])

    out1, grads1 = both_ways()
    _check("module, first parameters", ref, ref.want, dict(h=out1, **grads1))
    handle = seq.handle.value
    want2 = _restated(ref, _changed(rnn, 31), "the changed parameters")
    out2, grads2 = both_ways()
    assert seq.handle.value == handle
    _check("module, changed parameters", ref, want2, dict(h=out2, **grads2))
    _moved("module", out1, out2, want2)


def test_the_forward_follows_the_parameters_on_one_handle():
    """``lg_lstm_seq_load_device`` twice on one handle: the second pack replaces the first in every element of wp and bp."""
    ref = lc.reference(lc.FOLLOW)
    T, B, I, H = ref.shape
    lib = S._lib()
    rnn = copy.deepcopy(ref.rnn).to(DEV)
    handle = S._handle(lib, rnn)                              # create + the first load
    x, h0, c0, dh = ref.x.to(DEV), ref.h0.to(DEV), ref.c0.to(DEV), ref.dh.to(DEV)

    def both_ways():
        _, h_out = S._guarded(T * B * H)
        _, ws = S._guarded(5 * T * B * H)
        rc = lib.lg_lstm_seq_forward(handle, x.data_ptr(), x.stride(0), h0.data_ptr(), c0.data_ptr(), h_out.data_ptr(), ws.data_ptr(), T, B, S._stream())
        assert rc == 0, lib.lg_lstm_seq_last_error()
        torch.cuda.synchronize()
        ws_fwd = ws.clone()
        rc = lib.lg_lstm_seq_backward(handle, rnn.weight_hh_l0.data_ptr(), dh.data_ptr(), c0.data_ptr(), ws.data_ptr(), T, B, S._stream())
        assert rc == 0, lib.lg_lstm_seq_last_error()
        torch.cuda.synchronize()
        return _got(ref, h_out, ws_fwd, ws)

    first = both_ways()
    _check("handle, first load", ref, ref.want, first)
    want2 = _restated(ref, _changed(rnn, 32), "the changed parameters")
    ps =[getattr(rnn, n) for n in PARAMS]
    assert lib.lg_lstm_seq_load_device(handle, *[p.data_ptr() for p in ps], S._stream()) == 0, lib.lg_lstm_seq_last_error()
    second = both_ways()
    _check("handle, second load", ref, want2, second)
    _moved("handle", first["h"], second["h"], want2)
    assert lib.lg_lstm_seq_destroy(handle) == 0


# ---------------------------------------------------------------------------------------------------------------- f. weights x 3
@pytest.mark.parametrize("shape", lc.TIMES_THREE)
def test_weights_times_three_match_float64_forward_and_backward(shape):
    ref = lc.reference(shape, 3.0)
    _check_forward("forward, weights x 3", ref)
    _check_backward("backward, weights x 3", ref)
    _check_module("module, weights x 3", ref)


# ---------------------------------------------------------------------------------------------------------------- g. determinism
def test_forward_and_backward_are_bit_identical_from_run_to_run():
    ref = lc.reference(lc.REPEAT)
    (a, wa, _), (b, wb, _) = _raw(ref), _raw(ref)
    assert torch.equal(a["h_out"], b["h_out"]), "h_out"
    assert torch.equal(wa, wb), "the workspace after the forward"
    assert torch.equal(a["ws"], b["ws"]), "dG"
    for r in (a, b):
        assert r["lib"].lg_lstm_seq_destroy(r["handle"]) == 0
