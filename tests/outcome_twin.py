"""NumPy restatement of the outcome statistics of k_outcome_post (csrc/lg_game_outcome.h, include/legged_game_outcome.h) on top of
tests/game_twin.py: from ``game_twin.dones`` (``dist_xy``, ``prey_r``, ``pred_r``), the low-level env's ``reset_buf`` / ``time_out_buf`` and
the PRE-step ``curr_episode_step`` -> the five flags per env, the seven integers of the launch and the six float32 means.

The flags are those of the done envs and are not exclusive; ``steps`` of a done env is its post-increment episode step.  The counts are
integers, so they do not depend on any order; a mean is ONE float32 division of two integers converted to float32 (NumPy's division is
correctly rounded, the library's is the 2.5-ulp one: the tests allow 3 ulp)."""
import numpy as np

F = np.float32
COUNTS = ("episodes", "captured", "prey_out", "predator_out", "fell", "survived", "steps")
FLAGS = COUNTS[1:6]
MEANS = COUNTS[1:]


def flags(p, dn, ll_reset, ll_time_out):
    """-> dict of bool [N]: ``done`` and the five flags."""
    ll_reset, ll_time_out = np.asarray(ll_reset) != 0, np.asarray(ll_time_out) != 0
    captured = dn["dist_xy"] < F(p["capture_dist"])
    prey_out, predator_out = np.zeros_like(captured), np.zeros_like(captured)
    if p["env_radius"] >= 0:
        prey_out, predator_out = dn["prey_r"] > F(p["env_radius"]), dn["pred_r"] > F(p["env_radius"])
    f = dict(captured=captured, prey_out=prey_out, predator_out=predator_out, fell=ll_reset & ~ll_time_out, survived=ll_reset & ll_time_out)
    f["done"] = captured | prey_out | predator_out | ll_reset
    return f


def counts(f, curr_episode_step):
    """The seven integers of one launch, in the order of ``COUNTS`` (int64 [7])."""
    done = f["done"]
    steps = int((np.asarray(curr_episode_step, np.int64)[done] + 1).sum())
    return np.array([int(done.sum())] + [int(f[k].sum()) for k in FLAGS] + [steps], np.int64)


def means(c, previous=None):
    """The six float32 means of the counts ``c``; with no done env they stay ``previous`` (zeros when None)."""
    if int(c[0]) == 0:
        return np.zeros(6, F) if previous is None else np.array(previous, F, copy=True)
    return (c[1:].astype(F) / F(c[0])).astype(F)


def outcome(p, dn, ll_reset, ll_time_out, curr_episode_step, previous_means=None):
    """-> (flags dict, counts int64 [7], means float32 [6])."""
    f = flags(p, dn, ll_reset, ll_time_out)
    c = counts(f, curr_episode_step)
    return f, c, means(c, previous_means)
