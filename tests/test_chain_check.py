"""The case table of tests/test_gpu_chain_forward_edges.py (tests/chain_check.py) reaches the edges it claims, every row of it is
needed for that, its inputs take both ELU branches in every layer, and the bars it asserts with can tell right from wrong: on every
case the restated arithmetic of the kernel (what a correct kernel computes) is within a quarter of the output bar of the float64
module, and each planted error -- a dropped lo half in any one layer, a dropped input or hidden column, the second bias register set
dropped, two rows exchanged across the half boundary, a dead row's clamp gone to row 0 -- is at least 3 bars out somewhere.  Over the
table: the restatement is 0.022 .. 0.053 of the 1e-4 output bar (2.2e-6 .. 5.3e-6; torch's own float32 forward 6e-8 .. 3.5e-7); a
dropped lo half is 3.9 .. 11.0 bars out (the weakest: layer 2's on one case), a dropped input column 28 .. 911, a dropped hidden column
87 .. 737, the by2 biases 222 .. 881, exchanged rows 505 .. 5986, the clamp 1649 .. 5800 -- every planted error 3 bars or more out on
every case it applies to, so the project's bar stands and no tighter one is defined.  CPU only."""
import os
import re

import pytest
import torch

from tests import chain_check as cc
from tests import wide_learner_check as wl

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
IDS = [c.id for c in cc.CASES]


def table_shortfalls(cases):
    """What the table ``cases`` does not reach: a list of sentences, empty for cc.CASES."""
    out = []

    def need(ok, what):
        if not ok:
            out.append(what)

    nets = [(cc.k0s(i), i, o, c) for c in cases for i, o in c.nets]
    for k in (11, 15):
        mine = [c for c in cases if cc.case_k0s(c) == k]
        need({i for kk, i, _, c in nets if kk == k and len(c.nets) == 2 and c.shared} >= set(cc.WIDTHS[k]),
             f"<{k}>: the first and last width and each side of every quad boundary, on actor + critic of one table")
        need(len({cc.staging(i) for kk, i, _, _ in nets if kk == k}) == 7, f"<{k}>: seven ways to stage the last k-step")
        need({o for kk, _, o, _ in nets if kk == k} >= set(cc.OUTPUTS), f"<{k}>: every output count")
        need({o for kk, _, o, c in nets if kk == k and c.mb == 33} >= set(cc.NEW_OUTPUTS), f"<{k}>: every output count but 12 and 1 at mb = 33")
        need({c.mb for c in mine} >= set(cc.MBS), f"<{k}>: every mb")
        single = [c for c in mine if len(c.nets) == 1]
        need({c.nets[0][1] == 1 for c in single} == {True, False}, f"<{k}>: a single net as actor and as critic shape")
        need({c.nets[0][0] for c in single} >= {cc.K0S_OF[k][0], cc.K0S_OF[k][-1]}, f"<{k}>: a single net at each end of the width range")
        two = [c for c in mine if len(c.nets) == 2]
        need(any(c.shared for c in two), f"<{k}>: two nets on one tensor")
        need(any(not c.shared and c.nets[0][0] == c.nets[1][0] for c in two), f"<{k}>: two nets on separate tensors of one width")
        need(any(not c.shared and (c.nets[0][0] + 3) // 4 != (c.nets[1][0] + 3) // 4 for c in two), f"<{k}>: two nets of different ldx")
        need(any(c.gathered and c.mb >= 8 for c in mine) and any(not c.gathered for c in mine), f"<{k}>: a gather with repeats and rows = None")
        need(any(cc.workgroup_walk(c.mb, k)[4:] == (17, 1) for c in mine), f"<{k}>: 17 workgroups, the last with one live row")
    need(any(c.gathered and c.mb == 1 for c in cases) and any(not c.gathered and c.mb == 1 for c in cases), "one row, gathered and not")
    need(all(c.mb <= 1025 and len(c.nets) <= 2 for c in cases), "every case small")
    need(all(cc.takes_the_chain(c.nets) for c in cases), "every case takes the chain")
    need(len({c.id for c in cases}) == len(cases), "ids differ")
    return out


def test_the_table_reaches_what_it_claims():
    assert table_shortfalls(cc.CASES) == []
    assert len(cc.CASES) == 42
    assert all(cid in cc.BY_ID for cid in cc.ROW_PROBE_CASES + (cc.REPEAT,) + tuple(cc.BASE.values()))
    assert {cc.BY_ID[c].mb for c in cc.ROW_PROBE_CASES} == {33, 65, 1025} and {cc.case_k0s(cc.BY_ID[c]) for c in cc.ROW_PROBE_CASES} == {11, 15}
    assert all(cc.case_k0s(cc.BY_ID[v]) == k for k, v in cc.BASE.items())
    # what the suite ran before this table: 235 and 169 -- both staged the same way up to the padding -- and outputs 12 and 1
    assert cc.staging(235)[:2] == cc.staging(169)[:2] == (2, 1)
    assert [cc.staging(w)[:2] for w in cc.WIDTHS[11]] == [(1, 0), (2, 0), (2, 0), (2, 1), (2, 1), (2, 2), (2, 2)]
    cc.assert_1025_rows_walk_every_rotation()


@pytest.mark.parametrize("row", range(len(cc.CASES)), ids=IDS)
def test_every_row_of_the_table_is_needed(row):
    short = table_shortfalls(cc.CASES[:row] + cc.CASES[row + 1:])
    print(f"[observed] without {cc.CASES[row].id}: {short}")
    assert short, f"{cc.CASES[row].id} ({cc.CASES[row].why}) adds nothing the table test asks for"


def test_the_host_rule_is_the_wide_learners():
    cc.assert_the_host_rule()
    assert cc.takes_the_chain.__doc__ and "takes_generic_forward" in cc.takes_the_chain.__code__.co_names


def test_the_arithmetic_restated_is_the_kernels():
    """The constants and predicates chain_check restates, against the text of csrc/lg_policy.h and csrc/lg_learner.hip."""
    with open(os.path.join(REPO, "legged_games_gym_amd", "csrc", "lg_policy.h")) as f:
        src = f.read()
    for text in ("__builtin_amdgcn_exp2f(1.442695041f * x) - 1.0f", "row[hf] = blockIdx.x * 64 + 32 * hf + (lane & 31)", "if (!live[hf]) row[hf] = C.mb - 1;",
                 "const int wv = (wave + blockIdx.x) & 7;", "r0 = (blockIdx.x * 5) % K0S, r1 = (blockIdx.x * 5) & 15, r2 = (blockIdx.x * 3) & 15",
                 "k0 + 4 <= N.ldx ? o : N.x", "k0 + 8 <= N.ldx ? o + 4 : N.x", "const int a = 8 * ii + 4 * h + r;", "if (a < N.out_dim)",
                 "hi[i] = (__bf16)v[i]; lo[i] = (__bf16)(v[i] - (float)hi[i]);", "(row < out_dim && col < in_dim) ? Wt[(size_t)row * in_dim + col] : 0.0f"):
        assert text in src, text
    with open(os.path.join(REPO, "legged_games_gym_amd", "csrc", "lg_learner.hip")) as f:
        host = f.read()
    for text in ("n.dims[4] <= 16 && (k0s == 15 || k0s == 11)", "L.k0p = (n.dims[0] + 3) & ~3;", "const dim3 grid((mb + 63) / 64, n_nets)"):
        assert text in host, text
    assert cc.LOG2E == 1.442695041


def test_the_bars_are_the_projects_own():
    with open(os.path.join(REPO, "tests", "test_gpu_rl.py")) as f:
        src = f.read()
    assert re.search(r"1e-4", src) and re.search(r"3e-4", src)
    assert (cc.OUT_BAR, cc.GRAD_BAR, cc.GRAD_ABS) == (wl.OUT_TOL[1], wl.GRAD_TOL[1], wl.GRAD_ABS) == (1e-4, 3e-4, 1e-10)


@pytest.mark.parametrize("cid", IDS)
def test_both_elu_branches_and_the_restatement_is_inside_a_quarter_of_the_bar(cid):
    ref = cc.reference(cid)
    for n, (net64, x) in enumerate(zip(ref.refs, ref.xb)):
        wl.assert_both_elu_branches(net64, x.double(), f"{cid} net {n}")
    fig = cc.bars_out(cc.restated_outputs(cid), ref.want_out)
    print(f"[observed] {cid}: restatement {fig:.4f} of the output bar ({fig * cc.OUT_BAR:.2e}); torch float32 {ref.f32_out_err:.2e}")
    assert fig < 0.25, f"{cid}: the restated arithmetic is {fig:.3f} of the output bar from float64"
    if ref.inputs.rows is not None and ref.inputs.case.mb >= 8:
        rows = ref.inputs.rows
        assert int(rows.min()) == 0 and int(rows.max()) == ref.inputs.table_rows - 1 and len(set(rows.tolist())) < rows.numel()


@pytest.mark.parametrize("plant", cc.PLANTS)
def test_every_planted_error_is_at_least_three_bars_out_somewhere(plant):
    worst = {}
    for c in cc.CASES:
        if not any(cc.plant_applies(plant, net, c.mb) for net in c.nets):
            continue
        worst[c.id] = cc.bars_out(cc.restated_outputs(c.id, plant), cc.reference(c.id).want_out)
    assert worst, plant
    best = max(worst, key=worst.get)
    print(f"[observed] {plant}: {len(worst)} cases, {min(worst.values()):.2f} .. {worst[best]:.2f} bars ({best}); "
          f"{sum(v >= 3.0 for v in worst.values())} cases at 3 bars or more")
    assert worst[best] >= 3.0, (plant, worst)


def test_the_reference_is_shared():
    cid = cc.BASE[15]
    assert cc.reference(cid) is cc.reference(cid) and cc.inputs(cid) is cc.reference(cid).inputs
    ref = cc.reference(cid)
    assert all(p.grad is None for r in ref.refs for p in r.parameters()) and len(ref.want_grads) == 16
    one = cc.one_row_grads(ref, 3, [d[3] for d in ref.d_out])
    assert len(one) == 16 and all(a.shape == b.shape for a, b in zip(one, ref.want_grads))
    # a shared table is one tensor, separate ones are two
    assert ref.inputs.xs[0] is ref.inputs.xs[1]
    sep = cc.inputs("sep_235_235")
    assert sep.xs[0] is not sep.xs[1] and not torch.equal(sep.xs[0], sep.xs[1])
