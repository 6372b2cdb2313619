"""The case lists of tests/test_gpu_flat_learner.py (tests/flat_learner_check.py) reach the edges they claim, for 256 compute units and
for two other counts; and the loss-table helpers the wide and the flat GPU tests share produce inputs on both sides of every clip edge.
CPU only."""
import pytest
import torch

from tests import flat_learner_check as fl
from tests import wide_learner_check as wl

CUS = (256, 64, 304)


@pytest.mark.parametrize("cus", CUS)
def test_every_case_is_scheduled_as_derived(cus):
    """What mb_cases says about a case (tiles, workgroups, trips, idle groups) is what the restated host rule gives for its mb."""
    cases = fl.mb_cases(cus)
    assert len({c.id for c in cases}) == len(cases)
    assert {b: [c.id for c in cases if c.build == b] for b in fl.BUILDS} == fl.CASE_IDS      # the ids do not depend on the count
    for c in cases:
        slots, partials = fl.BUILDS[c.build]
        assert fl.schedule(c.mb, c.n_nets, slots, partials, cus) == (c.n_tiles, c.wgs, c.n_iter, c.idle), c
        assert c.mb >= 1 and c.idle >= 0 and fl.case(cus, c.id) == c


@pytest.mark.parametrize("cus", CUS)
def test_the_cases_reach_the_edges_they_are_listed_for(cus):
    cases = fl.mb_cases(cus)
    two = [c for c in cases if c.n_nets == 2]
    bwd, fwd = [c for c in two if c.build == "backward"], [c for c in two if c.build == "forward"]
    assert {1, 15, 16, 17} <= {c.mb for c in bwd} and {1, 17, 49, 65} <= {c.mb for c in fwd}
    assert {c.wgs for c in bwd} >= {1, 2, 7, 8, 9, 15, 16, 17, 25}                    # n_partials of k_mlp_reduce
    for k in fl.REDUCE_PARTIALS:                                                      # ... each with an idle slot and a ragged last tile
        c = fl.case(cus, f"backward2-partials{k}")
        assert (c.wgs, c.n_iter, c.idle, c.mb % fl.TILE) == (k, 1, 1, 13)
    assert {c.n_iter for c in bwd} == {1, 2, 3} and {c.n_iter for c in fwd} == {1, 2, 3}
    for build, slots in (("backward", 2), ("forward", 4)):
        t2, t3 = fl.case(cus, f"{build}2-trip2"), fl.case(cus, f"{build}2-trip3")
        assert t2.n_iter == 2 and t2.idle == t2.wgs * slots - 1                       # second trip: one live group
        assert t3.n_iter == 3 and 0 < t3.wgs * slots - t3.idle <= 3                   # third trip: a handful
        assert t2.wgs == t3.wgs == (min(cus // 2, fl.TRAIN_WGS) if build == "backward" else cus // 2)
    assert any(c.idle >= 1 and c.n_iter == 1 and c.wgs == 1 for c in bwd) and any(c.idle >= 1 and c.wgs == 1 for c in fwd)   # a wholly idle group
    one = [c for c in cases if c.n_nets == 1]
    assert {c.build for c in one} == {"forward", "backward"} and {c.n_iter for c in one} == {1, 2} and min(c.mb for c in one) == 1
    # partial-sum slices are capped at LG_TRAIN_WGS, the forward build's workgroups are not
    assert fl.case(cus, "backward1-trip2").wgs == min(cus, fl.TRAIN_WGS) and fl.case(cus, "forward1-trip2").wgs == cus


def test_the_largest_case_at_256_compute_units_stays_small():
    assert max(c.mb for c in fl.mb_cases(256)) < 20000


def test_the_host_rule_on_known_launches():
    """schedule() against launches worked out by hand from mlp_fill (256 CUs)."""
    assert fl.schedule(24576, 2, 2, True, 256) == (1536, 128, 6, 0)                   # the flat task's mini-batch: full trips only
    assert fl.schedule(24576, 2, 4, False, 256) == (1536, 128, 3, 0)
    assert fl.schedule(37, 2, 2, True, 256) == (3, 2, 1, 1)
    assert fl.schedule(4805, 1, 2, True, 256) == (301, 151, 1, 1)
    assert fl.schedule(1, 1, 4, False, 304) == (1, 1, 1, 3)
    assert fl.schedule(16 * 1217, 1, 2, True, 304) == (1217, 256, 3, 319)             # capped at 256 slices on a larger part


def test_the_width_tables():
    assert fl.ACTOR_INPUTS == (1, 3, 4, 17, 32, 44, 47, 48) and fl.OUTPUTS == (1, 2, 3, 4, 5, 12, 13, 16)
    assert fl.CRITIC_PAIRS == ((48, 17), (3, 44), (47, 47)) and fl.HIDDEN == (128, 64, 32)
    paths = {(i % 4 == 0, i % 16 == 0) for i in fl.ACTOR_INPUTS}
    assert paths == {(False, False), (True, False), (True, True)}                     # scalar, mixed, vector rows of the LDS image
    assert any(i <= 16 for i in fl.ACTOR_INPUTS) and any(16 < i <= 32 for i in fl.ACTOR_INPUTS)       # waves 1 / 2 without a live input column
    assert any(o < 4 for o in fl.OUTPUTS) and any(o & 3 for o in fl.OUTPUTS) and 16 in fl.OUTPUTS


def test_rows_with_duplicates():
    rows = fl.rows_with_duplicates(torch.Generator().manual_seed(0), 149, 400)
    assert rows.dtype == torch.int64 and rows.numel() == 149 and rows.unique().numel() == 149 - 49
    assert int(rows.min()) == 0 and int(rows.max()) == 399


@pytest.mark.parametrize("A", [1, 12, 16])
def test_the_placed_ratios_and_value_steps_are_not_degenerate(A):
    """loss_tables + place_ratios_and_value_steps on the CPU device: evaluated in float64 on the very mean / value they were placed
    from, the ratios and value steps satisfy assert_loss_inputs_not_degenerate, and lie where the helper says."""
    R, mb, clip = 400, 197, 0.2
    g = torch.Generator().manual_seed(A)
    t = wl.loss_tables(A, R, g, dev="cpu")
    assert all(v.dtype == torch.float32 and v.shape[0] == R for v in t.values())
    assert bool((t["old_sigma"] == t["old_sigma"][0]).all()) and (A == 1 or float(t["old_sigma"][0].std()) > 0.0)
    ix = torch.randperm(R, generator=g)[:mb]
    mu = t["old_mu"][ix] + 0.3 * torch.randn(mb, A, generator=g)
    std = 0.5 + 1.0 * torch.rand(A, generator=g)
    val = torch.randn(mb, 1, generator=g) * 0.3
    wl.place_ratios_and_value_steps(t, ix, mu, std, val, g, clip)
    assert t["old_lp"].shape == (R, 1) and t["old_lp"].dtype == torch.float32
    s, v, kl, ent, ratio, dv = wl.ppo_loss(mu.double(), std.double(), val.double(),
                                           *(t[k][ix].double() for k in ("actions", "old_lp", "old_mu", "old_sigma", "adv", "old_val", "ret")), clip, 1)
    wl.assert_loss_inputs_not_degenerate(ratio, dv, clip)
    wl.assert_loss_inputs_not_degenerate(ratio, dv, clip, margin=1e-2)
    assert 1 - 2 * clip - 0.021 < float(ratio.min()) and float(ratio.max()) < 1 + 2 * clip + 0.021
    assert float(dv.abs().max()) < 2 * clip + 0.021
    assert all(bool(torch.isfinite(x).all()) for x in (s, v, kl, ent))
