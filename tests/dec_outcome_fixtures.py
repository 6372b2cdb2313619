"""Shared inputs of the decentralised game's outcome-statistics tests (CPU and device), computed once per process: the seeded single-launch
cases with their twin results, and the inputs of the four-call sequence.  Everything here is NumPy; the device side is in
tests/test_gpu_dec_outcome.py."""
import functools

import numpy as np

from tests import dec_game_twin as dt
from tests import dec_outcome_twin as ot
from tests.dec_game_fixtures import synthetic_state

F = np.float32
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000, 4096)      # one thread; a wave edge and a workgroup edge on either side; 4 and 16 workgroups
TERMINATIONS = (0.0, -0.5)                              # rewards_prey.scales.termination x dt: absent, present
SEQ_N, SEQ_CALLS, SEQ_QUIET = 257, 4, 2                 # the sequence: envs, calls, the call in which no env is done
CARRIED = ("root_states", "dof_pos", "dof_vel", "predator_pos", "obs_prey", "curr_episode_step", "episode_length_buf", "episode_sums", "episode_means")


def time_outs(ll_reset, seed):
    """A seeded half of ``ll_reset``: the low-level resets that are time-outs."""
    return np.asarray(ll_reset, bool) & (np.random.default_rng(seed).random(len(ll_reset)) < 0.5)


def _case(n, termination, seed, force_ll_reset=False):
    p = dt.params(num_envs=n, seed=4321 + n, custom_origins=n % 2, scale_termination_prey_dt=termination)
    step = 70 + n
    s = synthetic_state(p, n, seed=seed, step=step)
    if force_ll_reset:
        s = dict(s, ll_reset=np.ones(n, bool))
    want, info = dt.post(p, s, step=step)
    dt.assert_margins(p, info)
    ll_time_out = time_outs(s["ll_reset"], seed=7 * n + 3)
    f, c, m = ot.outcome(info, s["ll_reset"], ll_time_out, s["curr_episode_step"])
    assert np.array_equal(f["done"], want["reset_buf"].astype(bool))
    return dict(p=p, step=step, s=s, ll_time_out=ll_time_out, want=want, info=info, flags=f, counts=c, means=m)


@functools.lru_cache(maxsize=None)
def case(n, termination):
    """-> dict(p, step, s, ll_time_out, want, info, flags, counts, means) of one seeded launch on ``n`` envs."""
    return _case(n, termination, seed=n + (1000 if termination != 0 else 0))


@functools.lru_cache(maxsize=None)
def single_done_case():
    """One env whose low-level env reset it: the n = 1 cases of ``case`` have no done env, this one has exactly one."""
    return _case(1, 0.0, seed=1, force_ll_reset=True)


def coverage():
    """Over the whole parametrisation, on the twin alone: (how often each flag occurs, envs that raise two flags at once, done envs without
    a flag, the smallest distance of a capture decision from its threshold)."""
    occurs, double, bare, margin = {k: 0 for k in ot.FLAGS}, 0, 0, np.inf
    for n in SIZES:
        for termination in TERMINATIONS:
            c = case(n, termination)
            f = c["flags"]
            raised = sum(f[k].astype(int) for k in ot.FLAGS)
            for k in ot.FLAGS:
                occurs[k] += int(f[k].sum())
            double += int((raised >= 2).sum())
            bare += int((f["done"] & (raised == 0)).sum())
            assert not (~f["done"] & (raised > 0)).any()
            margin = min(margin, float(np.min(np.abs(c["info"]["dist_xy"] - F(c["p"]["capture_dist"])))))
    return occurs, double, bare, margin


def sequence_inputs():
    """The per-call inputs of the four-call sequence at ``SEQ_N`` envs: -> (p, initial state dict, list of per-call dicts with ``p`` (the
    call's parameters), ``step``, ``command_pred``, ``ll_rew``, ``ll_reset``, ``ll_time_out``).  Everything in ``CARRIED`` goes from call to
    call.  In call ``SEQ_QUIET`` no env is done: no low-level reset, a capture distance of zero in that call's parameters (the entry points
    are stateless: the parameters travel by value with every launch), and nobody at the time limit -- the envs ``synthetic_state`` puts
    within two steps of it have run out, and were reset, in the calls before."""
    n = SEQ_N
    p = dt.params(num_envs=n, seed=99, custom_origins=1, scale_termination_prey_dt=-0.5)
    s = synthetic_state(p, n, seed=33, step=500)
    rng = np.random.default_rng(19)
    calls = []
    for k in range(SEQ_CALLS):
        cmd = dt.pre(p, np.zeros((n, 4), F), rng.uniform(-3.0, 3.0, (n, 2)).astype(F))[1]
        ll_reset = rng.random(n) < 0.1
        pk = p
        if k == SEQ_QUIET:
            ll_reset[:] = False
            pk = dict(p, capture_dist=0.0)
        calls.append(dict(p=pk, step=500 + k, command_pred=cmd, ll_rew=rng.uniform(-0.02, 0.05, n).astype(F), ll_reset=ll_reset,
                          ll_time_out=time_outs(ll_reset, seed=40 + k)))
    state = {k: s[k] for k in CARRIED + ("env_origins",)}
    return p, state, calls


def sequence_twin():
    """The sequence through the twin alone (the state carried by the twin) -> list of (counts, smallest capture margin) per call."""
    p, state, calls = sequence_inputs()
    rows = []
    for c in calls:
        s = dict(state, command_pred=c["command_pred"], ll_rew=c["ll_rew"], ll_reset=c["ll_reset"])
        out, info = dt.post(c["p"], s, step=c["step"])
        _, cnt, _ = ot.outcome(info, c["ll_reset"], c["ll_time_out"], s["curr_episode_step"])
        rows.append((cnt, float(np.min(np.abs(info["dist_xy"] - F(p["capture_dist"]))))))
        state = dict(state, **{k: out[k] for k in CARRIED})
    return rows
