"""tests/game_twin.py (the NumPy float32 restatement of csrc/lg_game.h) reproduces the reference's own ``HighLevelGame.step`` and
``LowLevelGame._reset_root_states`` as recorded in tests/golden/game_step.npz / game_reset.npz (tools/make_game_golden.py).

Flags, counters, the shifted history and everything that is copied, added or subtracted must be BIT-equal on every env; the reward may
differ by 4 ulp of its largest intermediate (torch's own rounding of the norm and of the sum in the fixture).  The inputs keep clear of the
three thresholds (angle / capture distance / radius) and of |rel| = 0; that is asserted first."""
import json
import os

import numpy as np
import pytest

from tests import game_twin as tw
from tests.game_fixtures import check_call, load, sequence_calls

F = np.float32


@pytest.mark.parametrize("tag", ["a", "b"])
def test_twin_reproduces_the_reference_step(golden_dir, tag):
    g = load(golden_dir, "game_step.npz")
    seen = {"visible": 0, "occluded": 0, "capture_only": 0, "ll_only": 0, "both": 0, "neither": 0, "radius": 0, "total": 0}
    calls = 0
    for k, p, s, out, info, ll_cmd, want in sequence_calls(g, tag):
        tw.assert_margins(p, info)                                                   # section 3 of the issue, before anything is compared
        np.testing.assert_array_equal(s["command"].view(np.uint32), want["command"].view(np.uint32))         # the clip block of step()
        np.testing.assert_array_equal(ll_cmd.view(np.uint32), want["command"][:, :4].view(np.uint32))
        assert (np.abs(g[f"{tag}_in_command"][k]) > 2.0).any() and (np.abs(g[f"{tag}_in_command"][k][:, 2]) > np.pi).any()
        np.testing.assert_array_equal(info["predator_integrated"].view(np.uint32), want["predator_integrated"].view(np.uint32))
        np.testing.assert_array_equal(info["visible"], want["sense_flag"] != 0)     # sense_predator's own return values
        np.testing.assert_array_equal(out["obs"][:, 9:12].view(np.uint32), want["sense_pos"].view(np.uint32))
        check_call(p, s, out, info, want)
        # the history really shifts: the three older slots of this call are the three newer slots the previous call left (reset envs: the fill)
        keep = ~out["reset_buf"]
        np.testing.assert_array_equal(out["obs"][keep, 0:9], s["obs"][keep, 3:12])
        assert (out["obs"][out["reset_buf"], 0:9] == F(100)).all() and (out["obs"][out["reset_buf"], 12:15] == 0).all()
        cap, lld = info["capture"], s["ll_reset"] != 0
        seen["visible"] += int(info["visible"].sum()); seen["occluded"] += int((~info["visible"]).sum()); seen["total"] += len(cap)
        seen["capture_only"] += int((cap & ~lld).sum()); seen["ll_only"] += int((lld & ~cap).sum()); seen["both"] += int((cap & lld).sum())
        seen["neither"] += int((~out["reset_buf"]).sum()); seen["radius"] += int(info["radius"].sum())
        calls += 1
    assert calls >= 3 and seen["total"] >= 3 * 512
    assert seen["visible"] >= seen["total"] / 4 and seen["occluded"] >= seen["total"] / 4, seen
    assert min(seen["capture_only"], seen["ll_only"], seen["both"], seen["neither"]) > 0, seen
    assert (seen["radius"] > 0) == (tag == "b"), seen


@pytest.mark.parametrize("custom", [0, 1])
def test_twin_reproduces_the_reference_root_reset(golden_dir, custom):
    g = load(golden_dir, "game_reset.npz")
    t = f"c{custom}"
    p = json.loads(str(g[f"{t}_params"]))
    assert p["custom_origins"] == custom
    ids = g[f"{t}_env_ids"]
    root, pred = tw.reset_root(p, g[f"{t}_env_origins"], g[f"{t}_u_root"], g[f"{t}_u_pred"])
    want_root, want_pred = g[f"{t}_root_states"], g[f"{t}_predator_pos"]
    np.testing.assert_array_equal(root[ids].view(np.uint32), want_root[ids].view(np.uint32))              # bit-equal given the recorded draws
    np.testing.assert_array_equal(pred[ids].view(np.uint32), want_pred[ids].view(np.uint32))
    rest = np.setdiff1d(np.arange(root.shape[0]), ids)
    np.testing.assert_array_equal(want_root[rest], g[f"{t}_in_root_states"][rest])                       # the other envs were left alone
    np.testing.assert_array_equal(want_pred[rest], g[f"{t}_in_predator_pos"][rest])
    # the recorded draws are the keyed streams of the two game purposes
    u_root, u_pred = tw.draws(int(g[f"{t}_seed"]), root.shape[0], int(g[f"{t}_step"]))
    np.testing.assert_array_equal(u_root, g[f"{t}_u_root"]); np.testing.assert_array_equal(u_pred, g[f"{t}_u_pred"])
    off = want_root[ids, :2] - want_pred[ids, :2]
    assert ((np.abs(off) >= 1.0 - 1e-5) & (np.abs(off) <= 10.0 + 1e-5)).all() and (np.sign(off[:, 0]) == np.sign(off[:, 1])).all()
    assert (want_pred[ids, 2] == F(0.3)).all()


def test_wrap_and_threshold_helpers():
    a = np.array([0.0, 3.0, -3.0, 3.2, -3.2, 7.0, -7.0, 6.2831855, np.pi], F)
    w = tw.wrap_to_pi(a)
    assert (w <= F(3.14159274)).all() and (w > -F(3.1415928)).all()
    np.testing.assert_allclose(np.sin(w.astype(np.float64)), np.sin(a.astype(np.float64)), atol=1e-6)
    np.testing.assert_allclose(np.cos(w.astype(np.float64)), np.cos(a.astype(np.float64)), atol=1e-6)
    # a predator straight ahead is visible, one straight behind is not and repeats the previous sensed position
    p = tw.params(num_envs=2)
    prey, quat = np.zeros((2, 3), F), np.tile(np.array([0, 0, 0, 1], F), (2, 1))
    pred = np.array([[2.0, 0.0, 0.0], [-2.0, 0.0, 0.0]], F)
    newest = np.full((2, 3), 7.0, F)
    sensed, visible, angle, rel, nrel = tw.sense(p, pred, prey, quat, newest)
    assert visible.tolist() == [True, False] and (sensed[0] == pred[0]).all() and (sensed[1] == 7.0).all()
