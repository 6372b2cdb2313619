"""-m gpu: the rollout kernel's arguments from launch to launch.

k_step<..., ROLL> (lg_rollout_policy) reads its uniform arguments inside every policy step: field by field from the kernarg segment and,
behind the physics, as host-filled blocks (PostArgs in csrc/lg_kernels.hip) built at each launch from the parameters and bindings then in
force.  Nothing may be left over from an earlier launch, and the blocks must say what the fields they replace say.

17 envs: two workgroups, the second with one live env and 15 clamped lanes.  T = 3, self-collision on and off.  Helpers and tolerances
are those of tests/test_gpu_rollout_oracle.py.

(a) two consecutive eager launches with lg_set_params between them, which changes only values the post-physics stretch reads (one reward
    scale, the observation-noise scales); the push step and two time-out resets fall inside the second launch; every step of both
    launches against the oracle under the parameters in force at that launch.
(b) the T-step launch against T lg_step_policy launches from the same snapshot.  The relation the parent commit (3ce0669) shows on MI355X
    is asserted: see RELATION below.
"""
import numpy as np
import pytest
import torch

from legged_games_gym_amd import capi
from tests.test_gpu_rollout_oracle import (NO_COMPARE, TOLS, _check_actor, _check_oracle_step, _flat_setup, _np, _restore, _snap, _storage)

pytestmark = pytest.mark.gpu

N, T = 17, 3
C1 = 745                      # counters 745..747 in the first launch, 748..750 in the second: the push step (750) is its last step
# what test (b) found on the parent commit: every storage array and every state buffer of the 3-step launch bit-equal to three
# lg_step_policy launches (both kernels run the same arithmetic per step on the same inputs).  Not compared: the float-atomic extras
# slots, which the two paths publish at different times, and obs_buf, which only the single-step kernel writes.
RELATION = "bit-equal"


def _setup(sc):
    robot, p, o, d, ac, fa = _flat_setup(N, sc)
    L = _np(d.buf["episode_length_buf"]).copy()
    L[:] = np.minimum(L, 900)                                          # no other time-out in the six steps
    L[3], L[N - 1] = 996, 995                                          # time out in step 5 (first workgroup) and step 6 (the partial one)
    d.buf["episode_length_buf"].copy_(torch.from_numpy(L).to(d.buf["episode_length_buf"].dtype))
    return robot, p, o, d, ac, fa


def _roll(d, fa, S, steps, counter):
    _restore(d, S)
    st = _storage(steps, N)
    d.rollout_policy(fa, st, counter, obs0=d.buf["obs_buf"])
    assert d.sim.device_status(True) == 0
    return {k: _np(v) for k, v in st.items()}, _snap(d)


def _states(d, fa, S0, counter):
    """S_0 .. S_T of a T-step launch from S0 (S_k: the final state of the k-step launch; its storage is a prefix of the T-step launch's)."""
    roll, S_T = _roll(d, fa, S0, T, counter)
    S = {0: S0, T: S_T}
    for k in range(1, T):
        st_k, S[k] = _roll(d, fa, S0, k, counter)
        for name, v in st_k.items():
            assert np.array_equal(v, roll[name][:k + 1 if name == "obs" else k]), (k, name)
    return roll, S


@pytest.mark.parametrize("sc", [True, False], ids=["sc_on", "sc_off"])
def test_rollout_launches_follow_set_params(sc):
    robot, p, o, d, ac, fa = _setup(sc)
    p1 = type(p).from_buffer_copy(p)
    p2 = type(p).from_buffer_copy(p)
    t_rew = capi.REWARD_TERMS.index("tracking_lin_vel")
    assert p.reward_slot[t_rew] >= 0 and p.reward_scale[t_rew] > 0 and p.add_noise and p.noise_lin_vel > 0
    p2.reward_scale[t_rew] = 3.0 * p.reward_scale[t_rew]
    for f in ("noise_lin_vel", "noise_ang_vel", "noise_gravity", "noise_dof_pos", "noise_dof_vel"):
        setattr(p2, f, 2.0 * getattr(p, f))
    assert bytes(p1) != bytes(p2)

    S0 = _snap(d)
    roll1, SA = _states(d, fa, S0, C1)
    stale, _ = _roll(d, fa, SA[T], T, C1 + T)                          # the second launch as it would be WITHOUT the new parameters
    d.sim.set_params(p2)
    roll2, SB = _states(d, fa, SA[T], C1 + T)
    d.sim.set_params(p1)
    # the change is visible, and only where it should be: rewards and observations, not the physics of the first step
    assert np.abs(roll2["rew"] - stale["rew"]).max() > 5 * TOLS["rew_tol"] and np.abs(roll2["obs"][1:] - stale["obs"][1:]).max() > 5 * TOLS["obs_tol"]
    assert np.array_equal(roll2["actions"][0], stale["actions"][0]) and np.array_equal(roll2["dones"][0], stale["dones"][0])
    # the second launch holds the push step and a time-out reset in each workgroup
    assert (C1 + T + T - 1) % p.push_interval == 0
    assert roll1["time_outs"].sum() == 0 and roll2["time_outs"][:, 3].any() and roll2["time_outs"][:, N - 1].any()
    assert roll2["dones"][:, 3].any() and roll2["dones"][:, N - 1].any()

    report = {}
    for params, roll, S, c in ((p1, roll1, SA, C1), (p2, roll2, SB, C1 + T)):
        o.sim.set_params(params)
        for t in range(T):
            _check_oracle_step(o, S[t], S[t + 1], roll["obs"][t], roll["obs"][t + 1], roll["actions"][t], roll["rew"][t], roll["dones"][t],
                               roll["time_outs"][t], c + t, N, report)
            _check_actor(ac, fa, roll["obs"][t], roll["mean"][t], roll["actions"][t], c + t, report)
    print(f"[observed] set_params between launches sc={sc}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(report.items())))


@pytest.mark.parametrize("sc", [True, False], ids=["sc_on", "sc_off"])
def test_rollout_launch_equals_single_step_launches(sc):
    robot, p, o, d, ac, fa = _setup(sc)
    C = C1 + T                                                         # push step and both time-outs inside the T steps
    L = _np(d.buf["episode_length_buf"]).copy()
    L[3], L[N - 1] = 999, 998
    d.buf["episode_length_buf"].copy_(torch.from_numpy(L).to(d.buf["episode_length_buf"].dtype))
    S0 = _snap(d)
    roll, S_T = _roll(d, fa, S0, T, C)
    assert roll["time_outs"][:, 3].any() and roll["time_outs"][:, N - 1].any()

    _restore(d, S0)
    worst = {}
    diff = lambda name, a, b: worst.__setitem__(name, max(worst.get(name, 0.0), float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())))
    for t in range(T):
        obs_t = _np(d.buf["obs_buf"]).copy()
        actions, mean = d.step_policy(fa, d.buf["obs_buf"], C + t)
        assert d.sim.device_status(True) == 0
        diff("obs_in", roll["obs"][t], obs_t)
        diff("actions", roll["actions"][t], _np(actions)); diff("mean", roll["mean"][t], _np(mean))
        diff("rew", roll["rew"][t], _np(d.buf["rew_buf"])); diff("obs", roll["obs"][t + 1], _np(d.buf["obs_buf"]))
        diff("dones", roll["dones"][t], _np(d.buf["reset_buf"])); diff("time_outs", roll["time_outs"][t], _np(d.buf["time_out_buf"]))
    S_single = _snap(d)
    for name, v in S_single.items():
        if name not in NO_COMPARE and name != "obs_buf":              # the rollout writes observations to its storage only (compared above)
            diff("state:" + name, _np(S_T[name]), _np(v))
    print(f"[observed] rollout launch against single-step launches sc={sc}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())))
    assert RELATION == "bit-equal"
    assert all(v == 0.0 for v in worst.values()), {k: v for k, v in worst.items() if v != 0.0}
