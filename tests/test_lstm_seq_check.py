"""The case table of tests/test_gpu_lstm_sequence_edges.py (tests/lstm_seq_check.py) reaches the edges it claims, every row of it is
needed for that, and the bars it asserts with measure something: on every case the float32 restatement (what a correct kernel
computes) is within a quarter of every bar, and a dropped input or hidden column, two exchanged rows, a zero ``c_{-1}``, a dropped
``dc`` carry and a dropped k row of ``dG . W_hh`` are at least ten bars out.  Over the table: the control is at most 0.095 of the gate
bar (I = 256; 0.080 with weights x 3), 0.070 of the ``h`` bar (I = 235) and 0.006 of the ``dG`` bar; the weakest planted backward error
is the dropped k row at (3, 4, 2, 224), 20.6 bars in ``dG`` -- and only 4.4 to 8.9 bars in the weight gradients, the sums over all rows
that were all the backward was compared through before; the weakest forward one is the dropped hidden column there, 669 bars in ``h``
and 1807 in the gates.  CPU only."""
import os
import re

import pytest
import torch

from tests import lstm_seq_check as lc
from tests import wide_learner_check as wl

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
RUNS = [(s, 1.0) for s in lc.SHAPES] + [(s, 3.0) for s in lc.TIMES_THREE]


def table_shortfalls(new, old=lc.OLD_SHAPES):
    """What the table ``new`` (with the sequence tests' ``old`` shapes beside it) does not reach: a list of sentences, empty for lc.SHAPES."""
    every, out = tuple(old) + tuple(new), []
    launches = {s: lc.launch(s) for s in every}

    def need(ok, what):
        if not ok:
            out.append(what)

    need({l.waves for l in launches.values()} == set(range(1, 9)), "every wave count 1 .. 8")
    need({(l.odd, l.tail) for l in launches.values()} == {(o, r) for o in (False, True) for r in range(4)}, "every (K parity, ksteps % 4) pair")
    need({lc.staging(s) for s in every} == {"one", "divides", "equal", "above", "below"}, "every staging regime")
    # x_dk == 0 only steers anything where a thread stages a second element; the old (24, 96, 256, 256) does, two rows at a time
    need(any(lc.staging(s) == "divides" and launches[s].n_x > launches[s].nthreads and launches[s].x_drow > 2 for s in new),
         "I dividing 2H with more elements than threads and more than two rows per stride")
    need(any(lc.staging(s) == "one" and launches[s].waves == 8 for s in new), "one input on 8 waves")
    above = {s[2] for s in new if lc.staging(s) == "above"}
    need({lc.ROUGH_OBS, lc.MAX_IN} <= above, "I > 2H with the rough task's 235 observations and with the largest I")
    need(any(s[2] == lc.FLAT_OBS and launches[s].waves == 4 for s in new), "the flat task's 48 observations into 128 units")
    need({s[1] for s in every} >= {1, 4, 31, 32, 33, 65}, "B in {1, 4, 31, 32, 33, 65}")
    need(any(launches[s].blocks == 3 and launches[s].last_rows == 1 for s in new), "three workgroups, the last with one live row")
    need(any(launches[s].blocks == 2 and launches[s].last_rows == 1 for s in new), "two workgroups, the last with one live row")
    need({s[0] for s in every} >= {1, 2, lc.UPDATE_T, 2 * lc.UPDATE_T}, "T of 1, 2, the update's 24 and 48")
    need(all(s[0] * s[1] * (s[2] + s[3]) <= 24 * 65 * 256 for s in new), "every new case small")
    need(all(s[3] % 32 == 0 and 32 <= s[3] <= 256 and 1 <= s[2] <= lc.MAX_IN for s in every), "every shape one lg_lstm_seq_create takes")
    need(all(l.fwd_lds <= 2 * 256 * 33 * 4 and l.bwd_lds <= 4 * 256 * 33 * 4 for l in launches.values()), "LDS blocks within the largest shape's")
    need(not set(new) & set(old), "no shape the sequence tests already run")
    return out


def test_the_table_reaches_what_it_claims():
    assert table_shortfalls(lc.SHAPES) == []
    assert len(lc.CASES) == len(set(lc.SHAPES)) == 13
    assert set(lc.TIMES_THREE) <= set(lc.SHAPES) and lc.TIMES_THREE == ((24, 33, 13, 96), (24, 65, 17, 160))
    assert lc.FOLLOW in lc.SHAPES and lc.REPEAT in lc.SHAPES and lc.launch(lc.REPEAT).blocks == 3
    # what the sequence tests ran before this table: 1, 2 and 8 waves, no tail of 3, no I >= 2H
    assert {lc.launch(s).waves for s in lc.OLD_SHAPES} == {1, 2, 8}
    assert 3 not in {lc.launch(s).tail for s in lc.OLD_SHAPES}
    assert {lc.staging(s) for s in lc.OLD_SHAPES} == {"one", "below", "divides"}


@pytest.mark.parametrize("row", range(len(lc.CASES)))
def test_every_row_of_the_table_is_needed(row):
    rest = lc.SHAPES[:row] + lc.SHAPES[row + 1:]
    short = table_shortfalls(rest)
    print(f"[observed] without {lc.SHAPES[row]}: {short}")
    assert short, f"{lc.SHAPES[row]} ({lc.CASES[row].why}) adds nothing the table test asks for"


def test_the_launch_arithmetic_is_the_kernels():
    """lc.launch against the text of csrc/lg_lstm_seq.hip, so that a change there is met here."""
    with open(os.path.join(REPO, "legged_games_gym_amd", "csrc", "lg_lstm_seq.hip")) as f:
        src = f.read()
    for text in ("s->ksteps = (num_in + hidden + 1) / 2", "const int groups = A.ksteps / 4;", "for (int s = 4 * groups; s < A.ksteps; s++)",
                 "x_drow = nthreads / I, x_dk = nthreads - x_drow * I", "nthreads = 2 * H", "dim3(2 * s->hidden)",
                 "(size_t)2 * ksteps * LG_LSTM_SEQ_LD * sizeof(float)", "(size_t)4 * hidden * LG_LSTM_SEQ_LD * sizeof(float)"):
        assert text in src, text
    l = lc.launch((24, 33, 13, 96))
    assert (l.waves, l.K, l.ksteps, l.groups, l.tail, l.nthreads, l.n_x, l.x_drow, l.x_dk, l.blocks, l.last_rows) == (3, 109, 55, 13, 3, 192, 416, 14, 10, 2, 1)
    assert lc.launch((24, 32, 39, 224)).last_rows == 32 and lc.launch((3, 4, 2, 224)).last_rows == 4


def test_the_bars_are_the_projects_own():
    with open(os.path.join(REPO, "tests", "test_gpu_recurrent.py")) as f:
        assert re.search(r"^TOL = 2e-5$", f.read(), re.M)
    with open(os.path.join(REPO, "tests", "test_gpu_lstm_sequence.py")) as f:
        assert re.search(r"^TOL = 2e-5$", f.read(), re.M)
    assert lc.TOL == 2e-5 and lc.GRAD_REL == wl.GRAD_TOL[0] == 1e-4 and wl.GRAD_ABS == 1e-10


@pytest.mark.parametrize("shape,scale", RUNS, ids=[f"{s}x{k:g}" for s, k in RUNS])
def test_the_bars_pass_the_right_arithmetic_and_fail_the_wrong_one(shape, scale):
    """reference() itself asserts that the restatement agrees with float64 ``nn.LSTM`` autograd."""
    r = lc.reference(shape, scale)
    T, B, I, H = shape
    w = r.want
    assert w.gates.shape == w.dG.shape == (T, B, 4 * H) and w.h.shape == w.c.shape == (T, B, H) and w.dG.dtype == torch.float64
    assert w.dw_ih.shape == (4 * H, I) and w.dw_hh.shape == (4 * H, H) and w.db.shape == (4 * H,)
    assert int(r.lengths[0]) == T and 1 <= int(r.lengths.min()) and int(r.lengths.max()) <= T
    assert float(r.h0.abs().min()) > 0.0 and float(r.c0.abs().min()) > 0.0
    dead = ~r.live
    assert not r.x[dead].any() and not r.dh[dead].any()
    assert T == 1 or B == 1 or bool(dead.any()), "no padded step in the case"
    assert float(w.dG[dead].abs().max() if dead.any() else 0.0) == 0.0, "dG of the reference is not exactly zero at a padded (t, row)"
    assert float(w.dG[r.live].abs().max()) > 0.0
    print(f"[observed] {shape} x {scale:g}: restatement against float64 nn.LSTM autograd: " + ", ".join(f"{k} {v:.1e}" for k, v in r.agreement.items()))

    ctrl = lc.fractions(r.ctrl, w, lc.FORWARD_QUANTITIES + lc.BACKWARD_QUANTITIES)
    print(f"[observed] {shape} x {scale:g}: float32 control, fractions of the bars: " + ", ".join(f"{k} {v:.4f}" for k, v in ctrl.items()))
    for name, fig in ctrl.items():
        assert fig < 0.25, f"the float32 control's {name} is {fig:.3f} of its bar"

    for fault in lc.FORWARD_FAULTS:
        if fault == "x_rows_exchanged" and B == 1:
            continue
        bad = lc.restate(r.params, r.x, r.h0, r.c0, r.dh, forward_fault=fault)
        figs = lc.fractions(bad, w, lc.FORWARD_QUANTITIES)
        print(f"[observed] {shape} x {scale:g}: {fault}: " + ", ".join(f"{k} {v:.1f}" for k, v in figs.items()) + " bars")
        assert figs["gates"] > 10.0 and figs["h"] > 10.0, (fault, figs)
    for fault in lc.BACKWARD_FAULTS:
        if fault == "dh_rec_rows_exchanged" and B == 1:
            continue
        if fault in ("dc_carry_dropped", "k_row_dropped", "dh_rec_rows_exchanged") and T == 1:
            continue                                          # nothing is carried back from a step that does not exist
        bad = lc.restate(r.params, r.x, r.h0, r.c0, r.dh, backward_fault=fault)
        figs = lc.fractions(bad, w, lc.BACKWARD_QUANTITIES)
        print(f"[observed] {shape} x {scale:g}: {fault}: " + ", ".join(f"{k} {v:.1f}" for k, v in figs.items()) + " bars")
        assert figs["dG"] > 10.0, (fault, figs)


def test_the_reference_is_shared_and_the_recipe_is_the_sequence_tests():
    shape = lc.SHAPES[0]
    assert lc.reference(shape) is lc.reference(shape) and lc.reference(shape, 3.0) is not lc.reference(shape)
    rnn, x, h0, c0, dh, lengths = lc.make_inputs(shape)
    r = lc.reference(shape)
    assert torch.equal(x, r.x) and torch.equal(dh, r.dh) and torch.equal(h0, r.h0) and torch.equal(c0, r.c0) and torch.equal(lengths, r.lengths)
    assert all(torch.equal(a, b) for a, b in zip(lc.params_of(rnn), r.params))
    with open(os.path.join(REPO, "tests", "test_gpu_lstm_sequence.py")) as f:
        src = f.read()
    assert "lc.make_inputs(shape, scale, saturate)" in src and "manual_seed(1000" not in src      # one definition of the recipe
    case = lc.as_case(r)
    assert case["want_h"] is r.want.h and len(case["want_grads"]) == 4
