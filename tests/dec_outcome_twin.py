"""NumPy restatement of the outcome statistics of k_dec_outcome (csrc/lg_dec_game_outcome.hip, include/legged_dec_game_outcome.h) on top of
tests/dec_game_twin.py: from ``dec_game_twin.post`` 's ``info`` (``capture``, ``time_out``, ``done``), the low-level env's ``reset_buf`` /
``time_out_buf`` and the PRE-step ``curr_episode_step`` -> the four flags per env, the six integers of the launch and the five float32 means.

The flags are those of the done envs and are not exclusive; ``steps`` of a done env is its post-increment episode step.  The counts are
integers, so they do not depend on any order; a mean is ONE float32 division of two integers converted to float32 (NumPy's division is
correctly rounded, the library's is the 2.5-ulp one: the tests allow 3 ulp)."""
import numpy as np

F = np.float32
COUNTS = ("episodes", "captured", "timed_out", "fell", "ll_timed_out", "steps")
FLAGS = COUNTS[1:5]
MEANS = COUNTS[1:]


def flags(info, ll_reset, ll_time_out):
    """-> dict of bool [N]: ``done`` and the four flags."""
    ll_reset, ll_time_out = np.asarray(ll_reset) != 0, np.asarray(ll_time_out) != 0
    f = dict(captured=np.asarray(info["capture"], bool), timed_out=np.asarray(info["time_out"], bool), fell=ll_reset & ~ll_time_out,
             ll_timed_out=ll_reset & ll_time_out)
    f["done"] = f["captured"] | f["timed_out"] | ll_reset
    assert np.array_equal(f["done"], np.asarray(info["done"], bool))
    return f


def counts(f, curr_episode_step):
    """The six integers of one launch, in the order of ``COUNTS`` (int64 [6])."""
    done = f["done"]
    steps = int((np.asarray(curr_episode_step, np.int64)[done] + 1).sum())
    return np.array([int(done.sum())] + [int((f[k] & done).sum()) for k in FLAGS] + [steps], np.int64)


def means(c, previous=None):
    """The five float32 means of the counts ``c``; with no done env they stay ``previous`` (zeros when None)."""
    if int(c[0]) == 0:
        return np.zeros(5, F) if previous is None else np.array(previous, F, copy=True)
    return (c[1:].astype(F) / F(c[0])).astype(F)


def outcome(info, ll_reset, ll_time_out, curr_episode_step, previous_means=None):
    """-> (flags dict, counts int64 [6], means float32 [5])."""
    f = flags(info, ll_reset, ll_time_out)
    c = counts(f, curr_episode_step)
    return f, c, means(c, previous_means)
