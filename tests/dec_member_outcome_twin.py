"""NumPy restatement of the outcome statistics per pool member of k_member_outcome (csrc/lg_member_outcome.hip, include/
legged_dec_game_member_outcome.h) on top of tests/dec_outcome_twin.py: the flags and the episode steps of the done envs, grouped by the pool
member of the env's 32-env block, ``clip(slot[e // 32], 0, count - 1)`` -> int64 ``[16, 6]`` in the order of ``dec_outcome_twin.COUNTS``.
Integers only: the rows do not depend on any order, and their column sums are the pooled counts of ``dec_outcome_twin.counts``."""
import numpy as np

from tests import dec_outcome_twin as ot

ROWS, BLOCK = 16, 32


def env_member(slots, n, count):
    """The pool member of every env: int64 [n]."""
    slots = np.asarray(slots, np.int64)
    assert slots.shape == ((n + BLOCK - 1) // BLOCK,) and 1 <= count <= ROWS
    return np.clip(slots, 0, count - 1)[np.arange(n) // BLOCK]


def member_counts(f, curr_episode_step, slots, count):
    """The six integers of one launch per member (int64 [16, 6]); ``f`` from ``dec_outcome_twin.flags``, the PRE-step ``curr_episode_step``."""
    done = f["done"]
    n = len(done)
    member = env_member(slots, n, count)
    steps = np.where(done, np.asarray(curr_episode_step, np.int64) + 1, 0)
    out = np.zeros((ROWS, len(ot.COUNTS)), np.int64)
    for m in range(ROWS):
        rows = member == m
        out[m] = [int((done & rows).sum())] + [int((f[k] & done & rows).sum()) for k in ot.FLAGS] + [int(steps[rows].sum())]
    assert np.array_equal(out.sum(axis=0), ot.counts(f, curr_episode_step))
    return out
