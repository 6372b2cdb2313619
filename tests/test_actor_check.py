"""The case table of tests/test_gpu_actor_edges.py (tests/actor_check.py) reaches the edges it claims, and the bars it asserts with
measure something: on every case the arithmetic a correct kernel does (float32; split-bf16 with the cross terms) passes with room, and
a lost cross term, one padded observation column too many and two exchanged action rows do not.  Over the table: float32 torch at
most 0.07 of the exact bar, the split-bf16 model at most 0.23 of the split bar, hi*hi alone at least 13.9 split bars.  CPU only."""
import os
import re

import pytest
import torch

from tests import actor_check as ac
from tests import wide_learner_check as wl

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))


def _of(kernel):
    return [c for c in ac.CASES if c.kernel is kernel]


def test_the_kernels_and_their_tile_ranges():
    assert [k.name for k in ac.KERNELS] == ["exact3", "exact15", "exact11", "exact2", "exact1", "wide15", "wide11", "wide2", "wide1"]
    assert {k.tiles: k.widths for k in ac.KERNELS} == {3: (33, 47, 48), 15: (225, 235, 240), 11: (161, 169, 176), 2: (17, 19, 32), 1: (1, 3, 16)}
    for k in ac.KERNELS:
        first, mid, last = k.widths
        assert first == 16 * (k.tiles - 1) + 1 and last == 16 * k.tiles and first < mid < last      # nearly empty and full last tile
        assert (k.build, k.wg_envs, k.envs[:4]) in (("exact", 16, (1, 15, 16, 17)), ("wide", 32, (1, 31, 32, 33)))
        assert k.hidden == (ac.FLAT_HIDDEN if k.tiles == 3 else ac.WIDE_HIDDEN)
        for w in k.widths:                                    # the restated dispatch sends every width of the range to this kernel
            for precision in ((0, 1) if k.precision is None else (k.precision,)):
                assert ac.kernel_for(k.hidden, w, precision) == k.name


def test_every_kernel_meets_every_edge():
    assert len(set(ac.CASE_IDS)) == len(ac.CASES) and 90 <= len(ac.CASES) <= 110
    for k in ac.KERNELS:
        cases = _of(k)
        assert {c.num_obs for c in cases} == set(k.widths)
        assert {c.num_actions for c in cases} == set(ac.ACTIONS) == {1, 4, 5, 12, 13, 16}
        assert {c.num_envs for c in cases} == set(k.envs)
        assert {c.regime for c in cases} == set(ac.REGIMES)
        assert {c.num_envs - k.wg_envs for c in cases} >= {-1, 0, 1} and 1 in {c.num_envs for c in cases}
        full = [c for c in cases if c.num_actions == 16 and ac.ragged(c)]           # the fourth action group on idle lanes ...
        assert {k.widths[0], k.widths[-1]} <= {c.num_obs for c in full}             # ... with the nearly empty and the full last tile
        assert any(ac.workgroups(c) > 1 for c in full)
        assert max(c.num_envs for c in cases) <= 1000


def test_the_wide_kernels_walk_every_rotation_of_the_weight_stream():
    for k in ac.KERNELS:
        if k.build != "wide":
            continue
        big = [c for c in _of(k) if c.num_envs > 33]
        assert big
        for c in big:
            assert -(-c.num_envs // 32) == 32 == ac.workgroups(c) and ac.ragged(c)
            assert len({(5 * b) % 32 for b in range(ac.workgroups(c))}) == 32 == len(ac.rotations(c))
            assert {b % 8 for b in range(ac.workgroups(c))} == set(range(8))                  # every tile share (wave + blk) % 8
        assert any(c.num_actions == 16 for c in big)


def test_the_refusals_follow_the_restated_dispatch():
    for hidden, num_obs in ac.REFUSED_AT_ACT:
        assert 1 <= num_obs <= 256 and ac.kernel_for(hidden, num_obs, 0) is None and ac.kernel_for(hidden, num_obs, 1) is None
    assert {o for h, o in ac.REFUSED_AT_ACT if h == ac.WIDE_HIDDEN} == {33, 160, 177, 224, 241}     # each neighbour of a served range
    assert {o for h, o in ac.REFUSED_AT_ACT if h == ac.FLAT_HIDDEN} == {32, 49}
    assert ac.kernel_for(ac.WIDE_HIDDEN, 32, 1) == "wide2" and ac.kernel_for(ac.WIDE_HIDDEN, 161, 0) == "exact11"
    assert [d for d in ac.REFUSED_AT_CREATE if d[0] > 256 or d[4] > 16 or any(x % 16 for x in d[1:4])] == list(ac.REFUSED_AT_CREATE)
    assert sorted({w for _, w in ac.REPACK}) == [1, 16, 17, 32, 33, 48, 161, 176, 225, 240] and len(ac.REPACK) == 18


def test_the_bars_are_the_projects_own():
    with open(os.path.join(REPO, "tests", "test_gpu_recurrent.py")) as f:
        assert re.search(r"^TOL = 2e-5$", f.read(), re.M)
    assert ac.EXACT_TOL == 2e-5 and ac.SPLIT_TOL == wl.OUT_TOL[1] == 1e-4


@pytest.mark.parametrize("cid", ac.CASE_IDS)
def test_the_bars_pass_the_right_arithmetic_and_fail_the_wrong_one(cid):
    """Both bars on every case, whichever kernel runs it.  reference() itself asserts that both ELU branches are live in every layer."""
    r = ac.reference(cid)
    exact, split = ac.EXACT_TOL * r.scale, ac.SPLIT_TOL * r.scale
    assert r.want.shape == (r.case.num_envs, r.case.num_actions) and r.want.dtype == torch.float64 and r.bar == (exact if r.case.kernel.build == "exact" else split)
    hihi = ac.max_err(ac.split_bf16_forward64(r.net, r.obs, cross=False), r.want)
    zeroed = ac.max_err(ac.zeroed_last_column(r.net, r.obs), r.want)
    swapped = ac.swapped_action_rows(r.net, r.obs)
    assert (swapped is None) == (r.case.num_actions == 1)
    swap_err = None if swapped is None else ac.max_err(swapped, r.want)
    print(f"[observed] {cid}: scale {r.scale:.3f}; float32 {r.f32_err / exact:.3f} of the exact bar; split-bf16 {r.emu_err / split:.3f}, hi*hi only "
          f"{hihi / split:.1f}, zeroed column {zeroed / split:.1f}, swapped rows {'-' if swap_err is None else f'{swap_err / split:.1f}'} of the split bar")
    assert r.f32_err < 0.25 * exact
    assert r.emu_err < 0.5 * split
    assert hihi > 10.0 * split
    assert zeroed > split > exact
    assert swap_err is None or swap_err > split


def test_the_reference_is_shared_and_the_inputs_are_reproducible():
    cid = ac.CASE_IDS[0]
    assert ac.reference(cid) is ac.reference(cid)
    c = ac.case(cid)
    net, obs, std = ac.make_inputs(c.num_obs, c.kernel.hidden, c.num_actions, c.num_envs, c.regime, c.seed)
    r = ac.reference(cid)
    assert torch.equal(obs, r.obs) and all(torch.equal(a, b) for a, b in zip(net.parameters(), r.net.parameters()))
    assert std.numel() == c.num_actions and (c.num_actions == 1 or float(std.diff().min()) > 0.0)
