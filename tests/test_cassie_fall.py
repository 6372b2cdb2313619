"""CPU, oracle only: Cassie's fall (tests/cassie_fall.py) does what the device test (tests/test_gpu_cassie_fall.py) relies on, and one
policy step from its states is well conditioned enough to be compared at the project's Cassie budget.  These are conditions on the
inputs, not kernel tolerances."""
import numpy as np
import pytest

from legged_games_gym_amd import capi
from tests import cassie_fall as F

N, T = F.N, F.T
TAIL = slice(F.WORKGROUP_ENVS, N)                # envs 32..39: the live lanes of the partial second workgroup


@pytest.mark.parametrize("kind", F.KINDS)
def test_the_fall_visits_every_branch(oracle_lib, kind):
    """Hard limits, the speed limit, one and two toes in the same step, base contact, resets in the partial workgroup and in its last
    env, no time-outs and, on the height field, terrain-level changes -- from the oracle's masks alone."""
    tr = F.trajectory(kind)
    st = lambda name: F.stacked(tr, name)
    toes, reset, base, level = st("toes"), st("reset"), st("base"), st("level")
    mixed = (toes == 1).any(axis=1) & (toes == 2).any(axis=1)
    print(f"[observed] {kind}: beyond a hard limit at step 1 {int(st('beyond_limit')[0].sum())}; env-steps ending at a speed limit {int(st('at_vel_limit').sum())}; "
          f"first contact at step {int(np.nonzero((toes > 0).any(axis=1))[0][0]) + 1}; steps with one- and two-toe envs {int(mixed.sum())}; all envs on both toes in steps "
          f"{(np.nonzero((toes == 2).all(axis=1))[0] + 1).tolist()}; one-toe env-steps {int((toes == 1).sum())}; base-contact env-steps {int(base.sum())}; resets {int(reset.sum())} "
          f"(first at step {int(np.nonzero(reset.any(axis=1))[0][0]) + 1}), in envs 32..39 {int(reset[:, TAIL].sum())}, env 39 at steps {(np.nonzero(reset[:, N - 1])[0] + 1).tolist()}; "
          f"level changes {int(level.sum())}, in envs 32..39 {int(level[:, TAIL].sum())}")
    assert st("beyond_limit")[0].sum() >= 5
    assert st("at_vel_limit").any()
    assert mixed.sum() >= 3
    assert (reset & base).sum() >= 10 and np.array_equal(reset, base)   # every reset is a base contact, and every base contact resets
    assert reset[:, TAIL].sum() >= 2 and reset[:, N - 1].any()
    assert not st("time_out").any()
    if kind == "heightfield":
        assert level.sum() >= 10 and level[:, TAIL].any()
        assert not (level & ~reset).any()
    else:
        assert not level.any()


@pytest.mark.parametrize("kind", F.KINDS)
def test_reset_envs_carry_the_termination_term(oracle_lib, kind):
    """rew_buf of every reset env holds reward_scale[TERMINATION] = -200 dt exactly: the same step from the same state with that one
    scale set to zero gives rew_buf' with rew_buf == rew_buf' + reward_scale[TERMINATION] in fp32, and the same rew_buf on every other env."""
    tr = F.trajectory(kind)
    s = F.fall_setup(kind)
    tid = capi.REWARD_TERMS.index("termination")
    scale = np.float32(s["p"].reward_scale[tid])
    assert scale == np.float32(-200.0 * s["p"].dt_policy) and s["p"].reward_slot[tid] >= 0
    s["p"].reward_scale[tid] = 0.0
    o = F.new_oracle(s)
    checked = 0
    for t in range(1, T + 1):
        reset = tr["events"][t - 1]["reset"]
        if not reset.any():
            continue
        F.load_state(o, tr["states"][t - 1])
        o.step(tr["actions"][t - 1], t)
        rew, rew0 = tr["states"][t]["rew_buf"], o.buf["rew_buf"]
        assert np.array_equal(o.buf["reset_buf"].astype(bool), reset)
        assert np.array_equal(rew[reset], rew0[reset] + scale) and np.array_equal(rew[~reset], rew0[~reset])
        assert (np.abs(rew[reset] - scale) < 0.15).all()                  # -4 dominates what else the step earned
        checked += int(reset.sum())
    assert checked >= 10


@pytest.mark.parametrize("kind", F.KINDS)
def test_one_step_from_every_state_is_well_conditioned(oracle_lib, kind):
    """The reference-only margin: each of the 48 steps again from its recorded state with root_states and dof_state scaled by
    1 + 1.2e-7 N(0, 1) (one fp32 ulp of input noise).  Every flag of all 1920 env-steps is unchanged -- so no reset, contact flag or level
    decision of this trajectory sits on a rounding edge -- and no env-step moves by more than pos 1e-3 / vel 0.1, half and a third of the
    budget the device is held to.
    [observed] worst over the 1920 env-steps: plane 6.0e-6 rad, 4.5e-4 rad/s (root pose 7.6e-6, root velocity 6.8e-5); height field
    4.9e-6 rad, 4.2e-4 rad/s (root pose 1.5e-5 -- an ulp of a 40 m coordinate is 3.8e-6 --, root velocity 6.3e-5).  Three more noise seeds
    gave the same flags and no figure above 1.05 times these."""
    tr = F.trajectory(kind)
    s = tr["setup"]
    o = F.new_oracle(s)
    rng = np.random.default_rng(5)
    worst = dict(pos=0.0, vel=0.0, root_pose=0.0, root_vel=0.0)
    for t in range(1, T + 1):
        F.load_state(o, tr["states"][t - 1])
        for k in ("root_states", "dof_state"):
            o.buf[k][...] = (o.buf[k].astype(np.float64) * (1.0 + 1.2e-7 * rng.standard_normal(o.buf[k].shape))).astype(np.float32)
        o.step(tr["actions"][t - 1], t)
        ref = tr["states"][t]
        for k in F.FLAGS:
            if k in ref:
                assert np.array_equal(o.buf[k], ref[k]), (k, t)
        q_o, q_r = o.buf["dof_state"].reshape(N, 12, 2).astype(np.float64), ref["dof_state"].reshape(N, 12, 2).astype(np.float64)
        r_o, r_r = o.buf["root_states"].astype(np.float64), ref["root_states"].astype(np.float64)
        e = dict(pos=np.abs(q_o[..., 0] - q_r[..., 0]).max(), vel=np.abs(q_o[..., 1] - q_r[..., 1]).max(),
                 root_pose=np.abs(r_o[:, :7] - r_r[:, :7]).max(), root_vel=np.abs(r_o[:, 7:] - r_r[:, 7:]).max())
        assert e["pos"] < 1e-3 and e["root_pose"] < 1e-3 and e["vel"] < 0.1 and e["root_vel"] < 0.1, (t, e)
        worst = {k: max(worst[k], float(e[k])) for k in worst}
    print(f"[observed] {kind}: worst over {T * N} env-steps " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
