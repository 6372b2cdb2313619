"""-m gpu: the three joint-level branches of the articulated-body passes, each driven on purpose, against the oracle.

The plane quadruped kernels take a joint's damping, armature and speed limit, the drive's torque at the joint's speed
(motor_torque) and the position-limit spring once per sub-step and hold them across both passes and the integrator
(csrc/lg_kernels.hip physics_substep, `HELD`).  No other test enters these branches on purpose: every ANYmal parity state is
far from the 20 rad/s speed limit, and ANYmal-C has no position limits at all.

N = 20: one full workgroup of 16 envs and a partial one with 4 live envs, whose dead lanes replicate env N - 1.  Every case sits in
env FIRST (first workgroup) and in env N - 1; every other env keeps the settled state (CONTROL is one of them) and is compared too.
anymal_c_flat starts from the state tests/test_gpu_rollout_oracle._flat_setup settles (self-collision on, and off), a1 from the
analogous plane setup (make_setup("a1", N, plane=True), 8 zero-action steps).

Each case first asserts from the ORACLE alone that its inputs do what they claim (conditions on inputs, not tolerances of the kernel):
(a) torque fade only.  LF_KFE at qd = -18.5 rad/s (0.925 v_lim) with tau = -1 N m (this direction lifts the foot; the other one drives
    it into the ground and the contact reverses the joint): tau qd > 0, 0.9 v_lim < |qd| < v_lim, |qd'| < v_lim, and qd' differs from
    the run with tau = 0.  [observed, oracle-settled state] qd' = -18.67 / -18.68 against -18.41 / -18.42 with tau = 0.
(b) speed-limit damper.  The same joint at qd = -10 with tau = -80: |qd'| == v_lim exactly, and an oracle whose model has no speed limit
    on that joint gives another qd' on the parent joint LF_HFE: the damper's reaction, not only the integrator's clamp, is in the result.
    The two case envs are lifted 0.05 m off the ground for this: standing, the foot's stick impedance keeps the joint under the limit in
    the first pass (the second pass, sliding, exceeds it), so the damper is never armed and only the clamp acts -- [observed] from the
    oracle-settled state the parent joint shows the reaction in 2 of 20 envs (10 and 17), not in env N - 1.  Lifted: [observed]
    qd' = -20.0 (-37.3 / -37.4 without the limit); LF_HFE 1.50 / 2.54 against 2.54 / 3.59 rad/s without.
(c) position limit.  a1, FL_thigh 0.03 rad beyond its upper limit in env FIRST and beyond its lower one in env N - 1: qd' points back
    into the range and differs by more than 1 rad/s from the same joint placed 0.03 rad inside.  [observed] -1.98 / +1.99 against
    +0.50 / +0.29.
(e) a speed between two joints' limits.  a1, FL_hip (v_lim 52.4) at 35 rad/s, above the 28.6 rad/s of the thigh next to it: the hip stays
    free (|qd'| < its own limit and the oracle without a limit on that joint gives the same qd').  A joint tested against its neighbour's
    limit would be braked here.
(d) control: env CONTROL is untouched in every case.

Then lg_physics_substep with the case's torques (k_physics<Anymal, plane, SC / !SC>) against the oracle's physics_substep, every env, with
the bounds of tests/test_gpu_compact_inertia.test_substep_with_self_collision_and_ground_contact_on_one_body (those of
tests/test_gpu_self_collision.test_substep_parity_with_crossed_legs).  Nothing new is bounded.

The policy-step legs (lg_step, lg_rollout_policy) are not run for (a) and (b): they need tau qd > 0 in the first sub-step, and ANYmal's
actuator network opposes a fast joint whatever the action.  Oracle, settled state, LF_KFE at qd = -18.5 / -10: first-sub-step torque
+54.8 / +49.1 N m with action 0, +40.7 / +40.4 with action -100 (the clip), +58.0 / +55.6 with action +3 -- never negative, so neither
the fade nor the damper is entered through a policy step from these states.

The tests pin behaviour, not an implementation: they pass on the library of the commit before the held terms as well.
"""
import numpy as np
import pytest
import torch

from tests.common import grid_origins, make_setup, randomize_env_params
from tests.test_gpu_rollout_oracle import _flat_setup, _np, _restore, _snap, _state_to_oracle

pytestmark = pytest.mark.gpu

N = 20
FIRST, CONTROL = 3, 5


def _oracle_without_speed_limit(task, joint, tweak=None):
    from oracle.oracle import OracleSim
    cfg, robot, p, names, model, w = make_setup(task, N, plane=True, tweak=tweak)
    assert model.dof_vel_limit[joint] > 0.0
    model.dof_vel_limit[joint] = 0.0
    return OracleSim(p, model, robot, w, threads=16)


@pytest.fixture(scope="module", params=[True, False], ids=["sc_on", "sc_off"])
def anymal(request):
    sc = request.param
    robot, p, o, d, ac, fa = _flat_setup(N, sc)
    kfe, hfe = list(robot.dof_names).index("LF_KFE"), list(robot.dof_names).index("LF_HFE")
    o_free = _oracle_without_speed_limit("anymal_c_flat", kfe, tweak=lambda c: setattr(c.asset, "self_collisions", 0 if sc else 1))
    assert o_free.params.self_collision == int(sc)
    return dict(sc=sc, o=o, d=d, o_free=o_free, S=_snap(d), kfe=kfe, hfe=hfe, vlim=float(o.model.dof_vel_limit[kfe]))


@pytest.fixture(scope="module")
def a1():
    from oracle.oracle import OracleSim
    from legged_games_gym_amd.device_sim import DeviceSim
    cfg, robot, p, names, model, w = make_setup("a1", N, plane=True)
    o = OracleSim(p, model, robot, w, threads=16)
    d = DeviceSim(p, model, robot, torch.device("cuda:0"), w)
    fr, dm = randomize_env_params(N, 5)
    d.buf["env_origins"].copy_(torch.from_numpy(grid_origins(N)))
    d.buf["friction_coeffs"].copy_(torch.from_numpy(fr)); d.buf["base_mass_delta"].copy_(torch.from_numpy(dm))
    d.reset_idx(torch.arange(N, dtype=torch.int32), 0)
    z = torch.zeros(N, 12, device="cuda")
    for it in range(1, 9):                                             # settle onto the plane
        d.step(z, it)
    hip, thigh = list(robot.dof_names).index("FL_hip_joint"), list(robot.dof_names).index("FL_thigh_joint")
    return dict(o=o, d=d, o_free=_oracle_without_speed_limit("a1", hip), S=_snap(d), hip=hip, thigh=thigh, model=model)


def _with_dof(d, S, edits):
    """The snapshot S with dof_state[env, joint, column] = value for every (env, joint, column, value) of edits."""
    _restore(d, S)
    dof = S["dof_state"].clone()
    v = dof.view(N, 12, 2)
    for e, j, c, x in edits:
        v[e, j, c] = float(x)
    d.buf["dof_state"].copy_(dof)
    return _snap(d)


def _oracle_substep(o, S0, tau):
    """(qd after one sub-step, contact forces) of oracle o from S0 with the torques tau"""
    _state_to_oracle(o, S0, _np(S0["obs_buf"]))
    o.physics_substep(tau, True)
    return o.buf["dof_state"].reshape(N, 12, 2)[..., 1].astype(np.float64).copy(), o.buf["contact_forces"].reshape(N, -1, 3).astype(np.float64).copy()


def _check_substep(o, d, S0, tau, tag):
    """lg_physics_substep against the oracle's physics_substep from S0, every env (the oracle is left holding its result)."""
    _, cf_o = _oracle_substep(o, S0, tau)
    qd0 = _np(S0["dof_state"]).reshape(N, 12, 2)[..., 1].astype(np.float64)
    _restore(d, S0)
    d.physics_substep(torch.from_numpy(tau), True)
    assert d.sim.device_status(True) == 0
    cf_d = _np(d.buf["contact_forces"]).reshape(N, -1, 3).astype(np.float64)
    q_o, q_d = o.buf["dof_state"].reshape(N, 12, 2).astype(np.float64), _np(d.buf["dof_state"]).reshape(N, 12, 2).astype(np.float64)
    dqd = np.abs(q_o[..., 1] - qd0).max(axis=1)
    err_v = np.abs(q_o[..., 1] - q_d[..., 1]).max(axis=1)
    ratio = err_v / (1.0 + dqd)
    e_pos = float(np.abs(q_o[..., 0] - q_d[..., 0]).max())
    e_root = float(np.abs(o.buf["root_states"] - _np(d.buf["root_states"])).max())
    f_scale = max(1.0, float(np.abs(cf_o).max()))
    e_f = float(np.abs(cf_o - cf_d).max())
    print(f"[observed] substep {tag}: velocity error / (1 + |dqd|) q99 {np.quantile(ratio, 0.99):.3g} max {ratio.max():.3g} (case envs "
          f"{ratio[FIRST]:.3g} / {ratio[N - 1]:.3g}, control {ratio[CONTROL]:.3g}), dof_pos {e_pos:.3g}, root {e_root:.3g}, contact force {e_f:.3g} of {f_scale:.3g}")
    assert np.quantile(ratio, 0.99) <= 2e-4 and ratio.max() <= 1e-3, (float(np.quantile(ratio, 0.99)), float(ratio.max()))
    assert e_pos < 2e-5
    assert e_root < 1e-3
    assert e_f < 1e-3 * f_scale, (e_f, f_scale)
    assert np.array_equal(np.abs(cf_o).sum(axis=(1, 2)) > 1.0, np.abs(cf_d).sum(axis=(1, 2)) > 1.0)
    return q_d[..., 1]


def _untouched(S0, S, env):
    return all(torch.equal(S0[k].reshape(N, -1)[env], S[k].reshape(N, -1)[env]) for k in ("dof_state", "root_states"))


def test_torque_fade_below_the_speed_limit(anymal):
    """(a): motor_torque's fade, the speed-limit damper not entered."""
    A = anymal
    o, d, j, vlim = A["o"], A["d"], A["kfe"], A["vlim"]
    envs = (FIRST, N - 1)
    S0 = _with_dof(d, A["S"], [(e, j, 1, -18.5) for e in envs])
    tau = np.zeros((N, 12), np.float32)
    for e in envs:
        tau[e, j] = -1.0
    qd = _np(S0["dof_state"]).reshape(N, 12, 2)[..., 1]
    qd_zero, _ = _oracle_substep(o, S0, np.zeros((N, 12), np.float32))
    qd_new, _ = _oracle_substep(o, S0, tau)
    print(f"[observed] oracle, torque fade sc={A['sc']}: qd' {qd_new[list(envs), j].tolist()} against {qd_zero[list(envs), j].tolist()} with zero torque")
    for e in envs:
        assert tau[e, j] * qd[e, j] > 0.0 and 0.9 * vlim < abs(qd[e, j]) < vlim
        assert abs(qd_new[e, j]) < vlim and qd_new[e, j] != qd_zero[e, j]
    assert _untouched(A["S"], S0, CONTROL)
    _check_substep(o, d, S0, tau, f"torque fade sc={A['sc']}")


def test_speed_limit_damper_and_its_reaction(anymal):
    """(b): the second pass runs with the damper towards -v_lim, and the parent joint feels it."""
    A = anymal
    o, d, j, hfe, vlim = A["o"], A["d"], A["kfe"], A["hfe"], A["vlim"]
    envs = (FIRST, N - 1)
    S_up = {k: v.clone() for k, v in A["S"].items()}
    for e in envs:
        S_up["root_states"][e, 2] += 0.05               # foot off the ground: nothing but the limit holds the joint back
    S0 = _with_dof(d, S_up, [(e, j, 1, -10.0) for e in envs])
    tau = np.zeros((N, 12), np.float32)
    for e in envs:
        tau[e, j] = -80.0
    qd_free, _ = _oracle_substep(A["o_free"], S0, tau)
    qd_new, _ = _oracle_substep(o, S0, tau)
    print(f"[observed] oracle, speed limit sc={A['sc']}: qd' {qd_new[list(envs), j].tolist()}, LF_HFE {qd_new[list(envs), hfe].tolist()} against "
          f"{qd_free[list(envs), hfe].tolist()} without the limit (LF_KFE then {qd_free[list(envs), j].tolist()})")
    for e in envs:
        assert abs(qd_new[e, j]) == vlim
        assert qd_new[e, hfe] != qd_free[e, hfe] and abs(qd_free[e, j]) > vlim
    assert _untouched(A["S"], S0, CONTROL)
    qd_dev = _check_substep(o, d, S0, tau, f"speed limit sc={A['sc']}")
    for e in envs:
        assert abs(qd_dev[e, j]) == vlim


def test_position_limit_spring(a1):
    """(c): FL_thigh beyond its upper limit in env FIRST, beyond its lower one in env N - 1."""
    o, d, j = a1["o"], a1["d"], a1["thigh"]
    lo, hi = float(a1["model"].dof_lower[j]), float(a1["model"].dof_upper[j])
    assert lo < hi
    tau = np.zeros((N, 12), np.float32)
    S_in = _with_dof(d, a1["S"], [(FIRST, j, 0, hi - 0.03), (N - 1, j, 0, lo + 0.03)])
    S0 = _with_dof(d, a1["S"], [(FIRST, j, 0, hi + 0.03), (N - 1, j, 0, lo - 0.03)])
    qd_in, _ = _oracle_substep(o, S_in, tau)
    qd_new, _ = _oracle_substep(o, S0, tau)
    print(f"[observed] oracle, position limit: qd' {qd_new[FIRST, j]:.4g} (beyond hi) / {qd_new[N - 1, j]:.4g} (beyond lo) against "
          f"{qd_in[FIRST, j]:.4g} / {qd_in[N - 1, j]:.4g} placed 0.03 rad inside")
    assert qd_new[FIRST, j] < 0.0 and qd_new[N - 1, j] > 0.0
    assert abs(qd_new[FIRST, j] - qd_in[FIRST, j]) > 1.0 and abs(qd_new[N - 1, j] - qd_in[N - 1, j]) > 1.0
    assert _untouched(a1["S"], S0, CONTROL)
    _check_substep(o, d, S0, tau, "position limit")


def test_a_speed_between_two_joints_limits_leaves_the_faster_joint_free(a1):
    """(e): FL_hip above the thigh's speed limit and below its own."""
    o, d, j, jn = a1["o"], a1["d"], a1["hip"], a1["thigh"]
    v_own, v_next = float(a1["model"].dof_vel_limit[j]), float(a1["model"].dof_vel_limit[jn])
    assert jn == j + 1 and v_next < 35.0 < 0.9 * v_own
    envs = (FIRST, N - 1)
    tau = np.zeros((N, 12), np.float32)
    S0 = _with_dof(d, a1["S"], [(e, j, 1, 35.0) for e in envs])
    qd_free, _ = _oracle_substep(a1["o_free"], S0, tau)
    qd_new, _ = _oracle_substep(o, S0, tau)
    print(f"[observed] oracle, hip at 35 rad/s: qd' {qd_new[list(envs), j].tolist()}")
    for e in envs:
        assert v_next < abs(qd_new[e, j]) < v_own and qd_new[e, j] == qd_free[e, j]
    assert _untouched(a1["S"], S0, CONTROL)
    _check_substep(o, d, S0, tau, "hip between two limits")
