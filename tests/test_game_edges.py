"""The designed threshold cases of tests/game_edges.py through the IEEE float32 twins (tests/game_twin.py, tests/dec_game_twin.py): what
tests/test_gpu_game_edges.py asserts of the seven post kernels holds for the references alone, so the inputs -- not the device -- are what
make the conditions reachable.  On top of that, here only: the twin's distances on the exact rows equal the hypotenuse bit for bit, and
the ladder conditions (share of rungs inside the band, decided rungs per side, exactly one flip)."""
import functools

import numpy as np
import pytest

from tests import dec_game_twin as dt
from tests import game_edges as ge
from tests import game_twin as tw

F = np.float32
STEP = 7


@functools.lru_cache(maxsize=None)
def twin(family, name):
    L = ge.launches()[name]
    if family == "game":
        return tw.post(tw.params(**L["over"]), ge.game_state(L["t"]), step=STEP)
    return dt.post(dt.params(**L["over"]), ge.dec_state(L["t"]), step=STEP)


def group(family, prefix):
    return [n for n in ge.names(family) if n.startswith(prefix)]


def test_the_table_is_small_ragged_and_leaves_every_predator_where_it_is_written():
    sizes = {n: L["t"]["prey"].shape[0] for n, L in ge.launches().items()}
    assert max(sizes.values()) == 6 * ge.FOV_RUNGS == sizes["fov_ladders"] and all(s % 256 for s in sizes.values()), sizes
    assert len(ge.exact_thresholds()) == 45 and len(set(float(T) for T in ge.exact_thresholds())) == 45
    for name, L in ge.launches().items():
        s, d = ge.game_state(L["t"]), ge.dec_state(L["t"])
        assert not s["command"].any() and not d["command_pred"].any(), name                 # zero predator velocity
        if name != "dec_truth":
            assert (L["t"]["ep_len"] == 5).all(), name
        if name not in ("dec_truth", "outcome_truth"):
            assert not L["t"]["ll_reset"].any(), name
    # every row whose visibility is asserted goes on and is at least 2 m away (the coincident rows of the degenerate launch aside)
    for family in ("game", "dec"):
        for name in ge.names(family):
            L, a = ge.launches()[name], ge.truth(ge.launches()[name], family)
            rows = L["t"]["vis_known"] & ~np.isnan(a["angle"])
            assert not a["done"][rows].any() and (a["dist"][rows] >= 2.0 - 1e-6).all(), name


@pytest.mark.parametrize("family", ["game", "dec"])
def test_exact_rows_have_their_known_answers_on_the_twin(family):
    """At equality not captured and not out, one float inside captured, one float outside out; the twin's root of a perfect square is exact."""
    names = group(family, "exact_")
    assert len(names) == (90 if family == "game" else 45)
    hyp = np.array(ge.hypotenuses())
    for name in names:
        L = ge.launches()[name]
        out, info = twin(family, name)
        ge.check(L, family, out, info)
        a = ge.truth(L, family)
        assert a["done_decided"].all()
        T = float(F(L["over"]["capture_dist"] if "capture" in name else L["over"]["env_radius"]))
        at = np.isclose(a["dist"], hyp[np.argmin(np.abs(hyp - T))], rtol=0, atol=0)          # the rows whose hypotenuse this launch's threshold sits on
        assert at.sum() == 8
        reset = out["reset_buf"][at]
        near = hyp[np.argmin(np.abs(hyp - T))]
        if "capture" in name:
            assert reset.all() if T > near else not reset.any(), name
        else:
            assert reset.all() if T < near else not reset.any(), name


@pytest.mark.parametrize("family,name", [("game", "ladder_capture"), ("game", "ladder_radius"), ("dec", "ladder_capture"), ("game", "fov_ladders"), ("dec", "fov_ladders")])
def test_ladders_are_decided_outside_the_band_and_flip_once_on_the_twin(family, name):
    L = ge.launches()[name]
    out, info = twin(family, name)
    flips = ge.check(L, family, out, info)
    inside = ge.ladder_conditions(L, family, flips)
    for lad in L["ladders"]:
        f = flips[lad["id"]]
        print(f"{family} {name} ladder {lad['id']} ({lad['quantity']}): {inside[lad['id']]} rungs of {int((L['t']['ladder'] == lad['id']).sum())} inside the band, "
              f"twin's flip {f['distance']:.3g} {f['unit']} from the float64 crossing")


def test_the_angle_band_is_near_2e_6_rad():
    """8 x the twin's worst angle error on the ladders; a thousand times tighter than the 2e-3 rad margin of the seeded states."""
    b = ge.angle_band()
    print(f"B_angle = {b:.3e} rad (the twin's worst angle error {b / ge.ANGLE_FACTOR:.3e} rad)")
    assert 8 * 1e-7 < b < 4e-6


@pytest.mark.parametrize("family", ["game", "dec"])
def test_known_angles_and_degenerate_rows_on_the_twin(family):
    for name in group(family, "known_") + ["degenerate"]:
        L = ge.launches()[name]
        out, info = twin(family, name)
        ge.check(L, family, out, info)
        assert not out["reset_buf"].any()
    n = len(ge._ranges())
    vis = lambda name: twin(family, name)[0]["obs" if family == "game" else "obs_prey"][:, 15] == 1
    assert vis("known_task")[:n].all() and not vis("known_task")[n:2 * n].any() and vis("known_task")[2 * n:5 * n].all()          # ahead, behind, ahead with a height difference
    assert vis("known_pi").all() and not vis("known_below_pi")[n:2 * n].any()                                                          # acos(-1) is float32 pi
    assert vis("known_zero")[:n].all() and not vis("known_zero")[n:].any()                                                             # only what is exactly ahead
    L = ge.launches()["degenerate"]
    _, info = twin(family, "degenerate")
    nan = np.isnan(info["angle"])
    assert nan[:3].all() and not vis("degenerate")[:3].any()                                  # 0/0: occluded
    assert vis("degenerate")[3:3 + n].all()                                                   # exactly along the heading at yaw 0: an argument of exactly 1
    share = float(nan[L["arbitrary"]].mean())
    print(f"{family}: the IEEE float32 twin turns {100 * share:.1f}% of the {ge.N_ARBITRARY} arbitrary-yaw rows along the heading into NaN (occluded)")
    assert 0.2 < share < 0.5 and np.array_equal(vis("degenerate")[L["arbitrary"]], ~nan[L["arbitrary"]])
    assert vis("degenerate")[-5:].tolist() == [True, True, False, False, True]               # z = w = 0: forward is +x


def test_truth_tables_on_the_twins():
    """All eight combinations of capture, time limit and low-level reset (dec) and the table over the five causes (outcome): flags, time-outs,
    the termination term and the counts of the outcome statistics against the twins' own."""
    from tests import dec_outcome_twin as dot
    from tests import outcome_twin as ot
    L = ge.launches()["dec_truth"]
    out, info = twin("dec", "dec_truth")
    ge.check(L, "dec", out, info)
    a = ge.truth(L, "dec")
    combos = {(bool(c), bool(t), bool(r)) for c, t, r in zip(a["captured"], a["time_out"], L["t"]["ll_reset"])}
    assert len(combos) == 8 and a["done_decided"].all()
    assert (a["termination"] != 0).sum() == 20 and ((a["termination"] != 0) == (a["captured"] & ~a["time_out"])).all()
    assert set(L["t"]["ep_len"].tolist()) == {ge.MAX_LEN - 1, ge.MAX_LEN}
    _, counts, _ = dot.outcome(info, L["t"]["ll_reset"], L["t"]["ll_time_out"], L["t"]["ep_step"])
    np.testing.assert_array_equal(counts, a["counts"])
    L = ge.launches()["outcome_truth"]
    out, info = twin("game", "outcome_truth")
    ge.check(L, "game", out, info)
    a = ge.truth(L, "game")
    combos = {tuple(bool(v) for v in row) for row in zip(a["captured"], a["prey_out"], a["pred_out"], a["fell"], a["ll_timed_out"])}
    assert len(combos) == 8 * 3 and a["done_decided"].all()
    _, counts, _ = ot.outcome(tw.params(**L["over"]), info, L["t"]["ll_reset"], L["t"]["ll_time_out"], L["t"]["ep_step"])
    np.testing.assert_array_equal(counts, a["counts"])
