"""Shared inputs of the tests of the outcome statistics per pool member (CPU and device), computed once per process: one seeded launch per
env count (``dec_outcome_fixtures._case`` under a seed chosen so that the per-member counts cannot pass empty, see ``coverage``), the slot
tables, and the twin's result per table.  Everything here is NumPy."""
import functools

import numpy as np

from tests import dec_member_outcome_twin as mt
from tests import dec_outcome_fixtures as of
from tests import dec_outcome_twin as ot

# one thread; a block edge on either side (31 / 32 / 33: at 33 a wave holds two members); a whole wave; a workgroup edge on either side; a
# second workgroup with a ragged last block (300 = 9 blocks + 12 envs); eight workgroups
SIZES = (1, 31, 32, 33, 64, 255, 256, 257, 300, 2000)
# n -> (seed of the state, termination scale x dt: absent and present in turn).  ``coverage`` holds under these seeds; tests/
# test_dec_member_outcome_abi.py checks that on the CPU.
SEEDS = {n: (n, -0.5 if i % 2 else 0.0) for i, n in enumerate(SIZES)}


@functools.lru_cache(maxsize=None)
def case(n):
    """-> the dict of ``dec_outcome_fixtures._case`` for ``n`` envs (p, step, s, ll_time_out, want, info, flags, counts, means)."""
    seed, termination = SEEDS[n]
    return of._case(n, termination, seed=seed)


def slot_tables(n):
    """-> list of (name, int32 table [ceil(n / 32)], count): all one member; a different member per block, cycling through 16; the same with
    values outside the pool (-3 and 99, which the kernel clamps to 0 and count - 1); the cycling table under count 1 (every block clamps to
    member 0) and under count 5 (members 5 .. 15 clamp to 4)."""
    blocks = (n + mt.BLOCK - 1) // mt.BLOCK
    cycle = (np.arange(blocks) % 16).astype(np.int32)
    wild = cycle.copy()
    wild[0::5], wild[1::5] = -3, 99
    return [("one", np.full(blocks, 3, np.int32), 16), ("cycle", cycle, 16), ("wild", wild, 16), ("count1", cycle, 1), ("count5", cycle, 5)]


@functools.lru_cache(maxsize=None)
def member_counts(n, name):
    c = case(n)
    table, count = next((t, k) for nm, t, k in slot_tables(n) if nm == name)
    return mt.member_counts(c["flags"], c["s"]["curr_episode_step"], table, count)


def coverage(n):
    """On the twin alone, under the cycling table: (per flag, the number of members under which it is raised; envs that raise two flags)."""
    c = case(n)
    rows = member_counts(n, "cycle")
    raised = sum(c["flags"][k].astype(int) for k in ot.FLAGS)
    return {k: int((rows[:, 1 + i] > 0).sum()) for i, k in enumerate(ot.FLAGS)}, int((raised >= 2).sum())
