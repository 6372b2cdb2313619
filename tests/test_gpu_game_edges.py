"""-m gpu: the seven kernels that run the post stage of the predator-prey games (csrc/lg_game_post.h, csrc/lg_dec_game_post.h) on the designed
threshold cases of tests/game_edges.py, held to the float64 answers there -- the assertions tests/test_game_edges.py makes of the float32 twins,
minus the single flip (inside the band either answer is allowed).  Every (kernel, launch) pair runs once and is shared by the tests."""
import functools

import numpy as np
import pytest

from tests import dec_game_twin as dt
from tests import dec_member_outcome_twin as mt
from tests import game_edges as ge
from tests import game_twin as tw
from tests import pursuer_twin as pt
from tests.test_gpu_dec_game import device_post as dec_device_post
from tests.test_gpu_dec_member_outcome import MemberLauncher
from tests.test_gpu_dec_outcome import Launcher as DecLauncher
from tests.test_gpu_game import device_post
from tests.test_gpu_outcome import Launcher
from tests.test_gpu_pursuer_game import device_pursuer_post

pytestmark = pytest.mark.gpu
STEP = 7
FAMILY = {"k_game_post": "game", "k_pursuer_post": "game", "k_outcome_post<false>": "game", "k_outcome_post<true>": "game",
          "k_dec_post": "dec", "k_dec_outcome": "dec", "k_member_outcome": "dec"}
KERNELS = tuple(FAMILY)
COUNTING = ("k_outcome_post<false>", "k_outcome_post<true>", "k_dec_outcome", "k_member_outcome")
# the scripted pursuer held still: a speed limit of 0 clamps every velocity to 0 (lg_pursuer_post refuses a gain of 0)
STILL = pt.pursuer_params(max_lin_vel=0.0, min_lin_vel=0.0)


def slots(n):
    return (np.arange((n + mt.BLOCK - 1) // mt.BLOCK) % mt.ROWS).astype(np.int32)


@functools.lru_cache(maxsize=None)
def device(kernel, name):
    """Launch ``name`` of tests/game_edges.py on ``kernel`` -> the twin's output layout, plus ``totals`` (and ``member_totals``) of a counting kernel."""
    L = ge.launches()[name]
    t = L["t"]
    if FAMILY[kernel] == "game":
        p, s = tw.params(**L["over"]), ge.game_state(t)
        if kernel == "k_game_post":
            return device_post(p, s, STEP)
        if kernel == "k_pursuer_post":
            out = device_pursuer_post(p, STILL, s, STEP)
            assert not out["predator_command"].any()
            return out
        call = dict(p=p, q=STILL, step=STEP, command=s["command"], ll_rew=s["ll_rew"], ll_reset=s["ll_reset"], ll_time_out=t["ll_time_out"])
        K = Launcher(s, [call], scripted=kernel == "k_outcome_post<true>")
        K.launch(0, counter_on_device=False)
        out = K.outputs()
        accum, ticket, _, out["totals"] = K.stats()
        assert not accum.any() and ticket == 0
        return out
    p, s = dt.params(**L["over"]), ge.dec_state(t)
    if kernel == "k_dec_post":
        return dec_device_post(p, s, STEP)
    call = dict(p=p, step=STEP, command_pred=s["command_pred"], ll_rew=s["ll_rew"], ll_reset=s["ll_reset"], ll_time_out=t["ll_time_out"])
    n = t["prey"].shape[0]
    K = DecLauncher(s, [call]) if kernel == "k_dec_outcome" else MemberLauncher(s, [call], slots(n), mt.ROWS)
    K.launch(0, counter_on_device=False)
    out = K.outputs()
    accum, extras, ticket, _, out["totals"] = K.stats()
    assert not accum.any() and not extras.any() and ticket == 0
    if kernel == "k_member_outcome":
        maccum, out["member_totals"] = K.member_stats()
        assert not maccum.any()
    return out


def checked(kernel, name):
    """The shared assertions on one launch, and -- where every decision of the launch is decided -- the outcome counts exactly."""
    L, family = ge.launches()[name], FAMILY[kernel]
    out = device(kernel, name)
    flips = ge.check(L, family, out)
    a = ge.truth(L, family)
    if kernel in COUNTING and a["done_decided"].all():
        np.testing.assert_array_equal(out["totals"], a["counts"], err_msg=f"{kernel} {name}")
        if kernel == "k_member_outcome":
            f = dict(done=a["done"], captured=a["captured"], timed_out=a["time_out"], fell=a["fell"], ll_timed_out=a["ll_timed_out"])
            np.testing.assert_array_equal(out["member_totals"], mt.member_counts(f, L["t"]["ep_step"], slots(len(a["done"])), mt.ROWS), err_msg=name)
    return out, flips, a


def visible(kernel, name):
    return device(kernel, name)["obs" if FAMILY[kernel] == "game" else "obs_prey"][:, 15] == 1


@pytest.mark.parametrize("kernel", KERNELS)
def test_exact_rows_have_their_known_answers(kernel):
    """Perfect-square distances with the threshold on the hypotenuse and one float to either side of it, at origin 0 and at 192 m: at equality
    not captured and not out, one float inside captured, one float outside out.  No band: every float32 intermediate is exact, so the
    device's root of a perfect square has to be that square's root."""
    names = [n for n in ge.names(FAMILY[kernel]) if n.startswith("exact_")]
    assert len(names) == (90 if FAMILY[kernel] == "game" else 45)
    for name in names:
        _, _, a = checked(kernel, name)
        assert a["done_decided"].all()


@pytest.mark.parametrize("kernel", KERNELS)
def test_ladders_are_decided_outside_the_band(kernel):
    """One float per rung across the capture distance and both radii, 257 bearings across either edge of the field of view at three yaws:
    outside B_dist = 4 ulp of the threshold / B_angle = 8 x the twin's worst angle error the decision is the float64 one.  Prints how far
    from the float64 crossing the device's decisions differ from it at most (-s)."""
    for name in ("ladder_capture", "ladder_radius", "fov_ladders"):
        if name not in ge.names(FAMILY[kernel]):
            continue
        _, flips, _ = checked(kernel, name)
        worst = {}
        for f in flips.values():
            worst[f["quantity"]] = max(worst.get(f["quantity"], 0.0), f["distance"])
            unit = f["unit"]
        band = f"{ge.B_DIST_ULP:g} ulp" if unit == "ulp" else f"{ge.angle_band():.3e} rad"
        print(f"{kernel} {name}: farthest rung decided against float64, per quantity: " + ", ".join(f"{q} {d:.3g} {unit}" for q, d in worst.items()) + f" (band {band})")


@pytest.mark.parametrize("kernel", KERNELS)
def test_known_angles_and_degenerate_geometry(kernel):
    """Dead ahead, dead behind (an acos argument of exactly -1: float32 pi, occluded one float below it), a zero field of view, 0/0, the
    predator exactly along the heading, the clamp of the yaw quaternion: flags of 0 or 1, no NaN in an observation, finite rewards."""
    for name in ("known_task", "known_pi", "known_below_pi", "known_zero", "degenerate"):
        out, _, _ = checked(kernel, name)
        assert not out["reset_buf"].any()
    n = len(ge._ranges())
    assert visible(kernel, "known_task")[:n].all() and not visible(kernel, "known_task")[n:2 * n].any() and visible(kernel, "known_task")[2 * n:5 * n].all()
    assert visible(kernel, "known_pi").all() and not visible(kernel, "known_below_pi")[n:2 * n].any()
    assert visible(kernel, "known_zero")[:n].all() and not visible(kernel, "known_zero")[n:].any()
    vis = visible(kernel, "degenerate")
    assert not vis[:3].any() and vis[3:3 + n].all() and vis[-5:].tolist() == [True, True, False, False, True]
    share = 1.0 - float(vis[ge.launches()["degenerate"]["arbitrary"]].mean())
    print(f"{kernel}: {100 * share:.1f}% of the {ge.N_ARBITRARY} arbitrary-yaw rows along the heading are occluded (the IEEE float32 twin: 35.6%)")


@pytest.mark.parametrize("kernel", KERNELS)
def test_truth_tables(kernel):
    """dec: capture x time limit x low-level reset (x low-level time-out): ``reset_buf`` and ``time_out_buf`` exact, the termination term paid
    for a capture without time-out only, the counts of ``k_dec_outcome`` / ``k_member_outcome`` exact.  game: the counts of ``k_outcome_post``
    over captured, prey out, predator out, fell and survived."""
    name = "outcome_truth" if FAMILY[kernel] == "game" else "dec_truth"
    out, _, a = checked(kernel, name)
    assert a["done_decided"].all() and np.array_equal(out["reset_buf"].astype(bool), a["done"])


@pytest.mark.parametrize("family", ["game", "dec"])
def test_kernels_that_share_a_body_agree_bit_for_bit(family):
    kernels = [k for k in KERNELS if FAMILY[k] == family]
    keys = ("reset_buf", "obs", "rew", "predator_pos", "root_states") if family == "game" else ("reset_buf", "time_out_buf", "obs_prey", "obs_pred", "rew_prey",
                                                                                                     "rew_pred", "predator_pos", "root_states")
    view = lambda a: a.view(np.uint8) if a.dtype == bool else a.view(np.uint32)
    for name in ge.names(family):
        first = device(kernels[0], name)
        for k in kernels[1:]:
            other = device(k, name)
            for key in keys:
                np.testing.assert_array_equal(view(other[key]), view(first[key]), err_msg=f"{k} {name} {key}")
        counting = [device(k, name)["totals"] for k in kernels if k in COUNTING]
        np.testing.assert_array_equal(counting[0], counting[1], err_msg=name)
