"""tests/dec_game_twin.py (the NumPy float32 restatement of csrc/lg_dec_game.hip) reproduces the reference's own ``DecHighLevelGame.step`` with
``LowLevelGame._reset_dofs / _reset_root_states`` as recorded in tests/golden/dec_game_step.npz (tools/make_dec_game_golden.py).

Flags, counters, the shifted history, the joints, root state, predator position, the predator's observation and everything that is copied, added or
subtracted must be BIT-equal on every env; the two rewards and the episode sums may differ by 4 ulp of their largest intermediate (torch's own
rounding of the norm and of the sums in the fixture); the episode means by the summation bound of ``dec_game_twin.means_bound``.  The inputs keep
clear of the thresholds (angle / capture distance) and of |rel| = 0; that is asserted first."""
import numpy as np
import pytest

from tests import dec_game_twin as dt
from tests.dec_game_fixtures import check_call, load, sequence_calls

F = np.float32


@pytest.mark.parametrize("tag", ["a", "t"])
def test_twin_reproduces_the_reference_step(golden_dir, tag):
    g = load(golden_dir)
    seen = {"visible": 0, "occluded": 0, "capture": 0, "time_out": 0, "ll_only": 0, "neither": 0, "total": 0, "terminal": 0}
    calls, carried = 0, None
    for k, p, s, out, info, ll_cmd, want in sequence_calls(g, tag):
        dt.assert_margins(p, info)                                                   # before anything is compared
        assert g[f"{tag}_env_origins"].shape[0] == 512
        for have, key in ((s["command_prey"], "command_prey"), (s["command_pred"], "command_pred"), (ll_cmd, "ll_commands")):        # the clip block of step()
            np.testing.assert_array_equal(have.view(np.uint32), want[key].view(np.uint32), err_msg=key)
        raw_prey, raw_pred = g[f"{tag}_in_command_prey"][k], g[f"{tag}_in_command_pred"][k]
        assert (np.abs(raw_prey[:, :2]) > 1.0).any() and (np.abs(raw_prey[:, 2]) > np.pi).any() and (np.abs(raw_pred) > 2.0).any()
        np.testing.assert_array_equal(info["predator_integrated"].view(np.uint32), want["predator_integrated"].view(np.uint32))
        np.testing.assert_array_equal(info["visible"], want["sense_flag"] != 0)     # prey_sense_predator's own return values
        np.testing.assert_array_equal(out["obs_prey"][:, 9:12].view(np.uint32), want["sense_pos"].view(np.uint32))
        carried = check_call(p, s, out, info, want, carried=carried)
        done = out["reset_buf"]
        # the history really shifts: the three older slots of this call are the three newer slots the previous call left (reset envs: the fill)
        np.testing.assert_array_equal(out["obs_prey"][~done, 0:9], s["obs_prey"][~done, 3:12])
        np.testing.assert_array_equal(out["obs_prey"][~done, 12:15], s["obs_prey"][~done, 13:16])
        assert (out["obs_prey"][done, 0:9] == F(100)).all() and (out["obs_prey"][done, 12:15] == 0).all()
        # reset envs: joints inside 0.5 .. 1.5 x default, at rest; counters and episode sums zeroed; the others untouched
        q0 = np.asarray(p["default_dof_pos"], F)
        ratio = want["dof_pos"][done] / q0
        assert ((ratio >= 0.5 - 1e-6) & (ratio <= 1.5 + 1e-6)).all() and (want["dof_vel"][done] == 0).all()
        np.testing.assert_array_equal(want["dof_pos"][~done], s["dof_pos"][~done]); np.testing.assert_array_equal(want["dof_vel"][~done], s["dof_vel"][~done])
        assert (want["episode_length_buf"][done] == 0).all() and (want["curr_episode_step"][done] == 0).all() and (want["episode_sums"][:, done] == 0).all()
        np.testing.assert_array_equal(want["episode_length_buf"][~done], s["episode_length_buf"][~done] + 1)
        # the recorded draws are the keyed streams of the three game purposes
        for have, key in zip(dt.draws(p["seed"], 512, int(g[f"{tag}_step"][k])), ("u_root", "u_pred", "u_dof")):
            np.testing.assert_array_equal(have, g[f"{tag}_{key}"][k])
        assert not done[0] and not info["visible"][0]                                 # env 0: occluded and alive (module docstring of the generator)
        assert (want["rew_pred"] <= 0).all() and (want["rew_prey"][~(info["capture"] & ~info["time_out"])] >= 0).all()
        cap, to, lld = info["capture"], info["time_out"], s["ll_reset"] != 0
        seen["visible"] += int(info["visible"].sum()); seen["occluded"] += int((~info["visible"]).sum()); seen["total"] += len(cap)
        seen["capture"] += int(cap.sum()); seen["time_out"] += int(to.sum()); seen["ll_only"] += int((lld & ~cap & ~to).sum()); seen["neither"] += int((~done).sum())
        seen["terminal"] += int((want["episode_sums"][2] != 0).sum()) + int((cap & ~to).sum())
        calls += 1
    assert calls >= (4 if tag == "a" else 2) and seen["total"] >= calls * 512
    assert seen["visible"] >= seen["total"] / 4 and seen["occluded"] >= seen["total"] / 4, seen
    assert min(seen["capture"], seen["time_out"], seen["ll_only"], seen["neither"]) > 0, seen
    assert (p["scale_termination_prey_dt"] != 0) == (tag == "t")


def test_time_outs_start_one_step_before_to_one_step_after_the_limit(golden_dir):
    g = load(golden_dir)
    L = 1000
    start = g["a_in0_episode_length_buf"]
    assert {L - 1, L, L + 1} <= set(start.tolist())
    to0, to1 = g["a_time_out_buf"][0], g["a_time_out_buf"][1]
    assert (to0 == (start + 1 > L)).all()                                              # L and L + 1 time out in the first call ...
    alive = (start == L - 1) & ~g["a_reset_buf"][0].astype(bool)
    assert alive.any() and to1[alive].all()                                            # ... L - 1 in the second, unless something else reset it first


def test_means_are_the_mean_of_the_reset_envs_sums(golden_dir):
    """extras["episode"] of the fixture = mean over the reset envs of (carried sum + this step's term) / 20 s, recomputed here in float64."""
    g = load(golden_dir)
    for k, p, s, out, info, _, want in sequence_calls(g, "t"):
        done = info["done"]
        ref = info["means_sums"].astype(np.float64).mean(axis=1) / 20.0
        assert (np.abs(want["episode_means"] - ref) <= dt.means_bound(p, info) + 1e-12).all()
        assert want["episode_means"][0] > 0 > want["episode_means"][1] and want["episode_means"][2] < 0
        assert done.sum() > 50
