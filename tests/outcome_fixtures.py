"""Shared inputs of the outcome-statistics tests (CPU and device), computed once per process: the seeded single-launch cases with their twin
results, and the inputs of the four-call sequence.  Everything here is NumPy; the device side is in tests/test_gpu_outcome.py."""
import functools

import numpy as np

from tests import game_twin as tw
from tests import outcome_twin as ot
from tests import pursuer_twin as pt
from tests.pursuer_fixtures import synthetic_state

F = np.float32
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000, 4096)      # one thread; a wave edge and a workgroup edge on either side; 4 and 16 workgroups
RADII = (-1.0, 2.5)                                     # off; on, small enough that predators (within 2.83 m of their origin) leave it too
SEQ_N, SEQ_CALLS, SEQ_QUIET = 257, 4, 2                 # the sequence: envs, calls, the call in which no env is done


def time_outs(ll_reset, seed):
    """A seeded subset of ``ll_reset``: the low-level resets that are time-outs."""
    return np.asarray(ll_reset, bool) & (np.random.default_rng(seed).random(len(ll_reset)) < 0.5)


@functools.lru_cache(maxsize=None)
def case(n, radius):
    """-> dict(p, q, step, s, s_plain, ll_time_out, want, info, flags, counts, means) of one seeded launch on ``n`` envs.  ``s`` feeds the
    scripted variant.  ``s_plain`` is ``s`` with the pursuer's velocity in columns 4:6 of the command (it is within the clip range), so the
    plain variant moves the predator to the same place and the same twin results -- and the same threshold margins -- hold for both."""
    p, q = tw.params(num_envs=n, seed=4321 + n, env_radius=radius, custom_origins=n % 2), pt.pursuer_params()
    step = 70 + n
    s = synthetic_state(p, q, n, seed=n + (1000 if radius >= 0 else 0), step=step)
    want, info = pt.post(p, q, s, step=step)
    tw.assert_margins(p, info)
    command = s["command"].copy()
    command[:, 4:6] = info["predator_command"]
    s_plain = dict(s, command=command)
    plain_want, plain_info = tw.post(p, s_plain, step=step)
    assert np.array_equal(plain_info["dist_xy"], info["dist_xy"]) and np.array_equal(plain_want["reset_buf"], want["reset_buf"])
    ll_time_out = time_outs(s["ll_reset"], seed=7 * n + 3)
    f, c, m = ot.outcome(p, info, s["ll_reset"], ll_time_out, s["curr_episode_step"])
    assert np.array_equal(f["done"], want["reset_buf"].astype(bool))
    return dict(p=p, q=q, step=step, s=s, s_plain=s_plain, ll_time_out=ll_time_out, want=want, info=info, flags=f, counts=c, means=m)


def coverage():
    """Over the whole parametrisation, on the twin alone: (how often each flag occurs, envs that raise two flags at once, done envs without a flag)."""
    occurs, double, bare = {k: 0 for k in ot.FLAGS}, 0, 0
    for n in SIZES:
        for radius in RADII:
            f = case(n, radius)["flags"]
            raised = sum(f[k].astype(int) for k in ot.FLAGS)
            for k in ot.FLAGS:
                occurs[k] += int(f[k].sum())
            double += int((raised >= 2).sum())
            bare += int((f["done"] & (raised == 0)).sum())
            assert not (~f["done"] & (raised > 0)).any()
    return occurs, double, bare


def sequence_inputs(scripted):
    """The per-call inputs of the four-call sequence at ``SEQ_N`` envs: -> (p, q, initial state dict, list of per-call dicts with
    ``p`` (the call's parameters), ``step``, ``command``, ``ll_rew``, ``ll_reset``, ``ll_time_out``).  Root states, predator, observations
    and the episode counters are carried from call to call.  In call ``SEQ_QUIET`` no env is done: no low-level reset, and a capture
    distance of zero in that call's parameters (the entry points are stateless: the parameters travel by value with every launch)."""
    n = SEQ_N
    p, q = tw.params(num_envs=n, seed=99, env_radius=-1.0, custom_origins=1), pt.pursuer_params()
    s = synthetic_state(p, q, n, seed=31 if scripted else 32, step=500)
    rng = np.random.default_rng(17 if scripted else 18)
    calls = []
    for k in range(SEQ_CALLS):
        cmd = rng.uniform(-3.0, 3.0, (n, 6)).astype(F)
        ll_reset = rng.random(n) < 0.1
        pk = p
        if k == SEQ_QUIET:
            ll_reset[:] = False
            pk = dict(p, capture_dist=0.0)
        calls.append(dict(p=pk, step=500 + k, command=tw.pre(p, cmd)[0], ll_rew=rng.uniform(-0.02, 0.05, n).astype(F), ll_reset=ll_reset,
                          ll_time_out=time_outs(ll_reset, seed=40 + k)))
    state = {k: s[k] for k in ("root_states", "env_origins", "predator_pos", "obs", "curr_episode_step", "episode_length_buf", "episode_sums")}
    return p, q, state, calls


def sequence_twin(scripted):
    """The sequence through the twin alone (the state carried by the twin) -> list of (counts, smallest capture margin) per call."""
    p, q, state, calls = sequence_inputs(scripted)
    rows = []
    for c in calls:
        s = dict(state, command=c["command"], ll_rew=c["ll_rew"], ll_reset=c["ll_reset"])
        out, info = pt.post(c["p"], q, s, step=c["step"]) if scripted else tw.post(c["p"], s, step=c["step"])
        _, cnt, _ = ot.outcome(c["p"], info, c["ll_reset"], c["ll_time_out"], s["curr_episode_step"])
        rows.append((cnt, float(np.min(np.abs(info["dist_xy"] - F(c["p"]["capture_dist"]))))))
        state = dict(state, **{k: out[k] for k in ("root_states", "predator_pos", "obs", "curr_episode_step", "episode_length_buf", "episode_sums")})
    return rows
