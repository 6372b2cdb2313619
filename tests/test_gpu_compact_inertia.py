"""-m gpu: a limb body that carries a self-collision record AND a ground contact in the same final pass, against the oracle.

The rigid-body wave keeps each body's rigid inertia in its compact form (ten numbers, csrc/lg_device.h `RI`) and writes the 21 entries
out at the head of every inward step; in the final pass the self-collision records of body j are folded into that expansion inside
the inward loop, between the expansion and the body's ground contacts (csrc/lg_kernels.hip `self_fold`).  The order of accumulation
-- rigid terms, then self-collision terms, then ground contacts -- matters only where one body has both kinds of contact at once, and
no other test has that inside the fused kernels: tests/test_gpu_self_collision.py's crossed legs are airborne, and its policy step runs
lg_step only.

anymal_c_flat, N = 20 (one full workgroup of 16 envs and a partial one with 4 live envs, whose dead lanes replicate env N - 1),
self-collision on, and off as a control (the compact path without records).  From the settled state of
tests/test_gpu_rollout_oracle._flat_setup, envs 2, 7, 12 and N - 1 get LF_HAA / RF_HAA = q0 + S_SCALE (qx - q0) with qx of
tests/test_oracle_physics._crossing_pose: their front legs overlap while they stand on them.  Every other env keeps its state.

Each case first asserts from the ORACLE alone (one physics_substep with zero torques from that state) that the inputs are what they
claim: equal and opposite forces of more than 50 N on LF_THIGH / RF_THIGH of a crossed env, |f_y| > 50 N on a front foot (rigid
with the shank, the last body of the chain) of a crossed env, that foot loaded with f_z > 10 N from the ground by an oracle without
self-collision, no thigh force in an untouched env, and env N - 1 among the crossed ones.  Those are conditions on the inputs, not
tolerances of the kernel.  Chosen on the CPU with the oracle settling itself (8 zero-action steps), S_SCALE = 1.15:
[observed] thigh-pair forces of 128 - 528 N in all four crossed envs (|f_L + f_R| = 0), lateral front-foot forces of 3.4 - 7.3 kN, the
same feet carrying f_z = 420 - 1130 N without self-collision, no thigh force elsewhere; S_SCALE = 1.0 overlaps env 2 only (28 N).
From the device-settled state the test starts from: [observed] thigh pairs 535.7 / 140.4 / 385.7 / 405.5 N (envs 2, 7, 12, 19),
front-foot |f_y| 3.45 - 7.35 kN (env 7: its right foot has left the ground, 0 N), the same feet's f_z without self-collision
236 - 1126 N, 0 N on every other env's thighs.  Kernel against oracle (same figures with the library of the commit before the compact
inertia and with this one): sub-step velocity error / (1 + |dqd|) 1.7e-5 (bound 2e-4), contact force 0.016 N of 7.3 kN; policy
steps dof_vel 6.4e-5, obs 7.2e-6, rew 8e-8.

Then, with the existing tolerances: the device's physics_substep against the oracle's (k_physics<Anymal, plane, SC>; bounds of
tests/test_gpu_self_collision.test_substep_parity_with_crossed_legs), and lg_step with fixed actions, lg_step_policy and every step of
a 3-step lg_rollout_policy launch through tests/test_gpu_rollout_oracle._check_oracle_step with its TOLS.
"""
import numpy as np
import pytest
import torch

from tests.common import make_setup
from tests.test_gpu_rollout_oracle import C0, _check_oracle_step, _flat_setup, _launch, _np, _restore, _snap, _state_to_oracle
from tests.test_oracle_physics import _crossing_pose

pytestmark = pytest.mark.gpu

N = 20
STEPS = 3
CROSSED = (2, 7, 12, N - 1)
S_SCALE = 1.15
ACTION_SCALE = 0.3


@pytest.fixture(scope="module")
def oracle_without_self_collision():
    from oracle.oracle import OracleSim
    cfg, robot, p, names, model, w = make_setup("anymal_c_flat", N, tweak=lambda c: setattr(c.asset, "self_collisions", 1))
    assert p.self_collision == 0
    return OracleSim(p, model, robot, w, threads=16)


@pytest.fixture(scope="module", params=[True, False], ids=["sc_on", "sc_off"])
def settled(request):
    robot, p, o, d, ac, fa = _flat_setup(N, request.param)
    return request.param, robot, p, o, d, fa, _snap(d)


def _cross(d, S, robot, p):
    """The settled state with the front legs of the envs of CROSSED swung into each other; they do not time out within the checked steps."""
    _restore(d, S)
    q0 = np.array(list(p.default_dof_pos)[:12], np.float64)
    qx, sign, (lf, rf) = _crossing_pose(robot, q0)
    dof, ep = S["dof_state"].clone(), S["episode_length_buf"].clone()
    q = dof.view(N, 12, 2)
    for e in CROSSED:
        for j in (lf, rf):
            q[e, j, 0] = float(q0[j] + S_SCALE * (qx[j] - q0[j]))
        ep[e] = 10
    d.buf["dof_state"].copy_(dof); d.buf["episode_length_buf"].copy_(ep)
    return _snap(d)


def _substep(o, S0):
    _state_to_oracle(o, S0, _np(S0["obs_buf"]))
    o.physics_substep(np.zeros((N, 12), np.float32), True)
    return o.buf["contact_forces"].reshape(N, -1, 3).astype(np.float64).copy()


def _assert_inputs(sc, robot, o, o_off, S0):
    """From the oracle alone: the first sub-step from S0 has a self-collision record and a ground contact on the same leaf body."""
    bn = list(robot.body_names)
    crossed = np.zeros(N, bool)
    crossed[list(CROSSED)] = True
    assert crossed[N - 1]
    cf_off = _substep(o_off, S0)
    feet = [bn.index("LF_FOOT"), bn.index("RF_FOOT")]
    thighs = [i for i, n in enumerate(bn) if "THIGH" in n]
    fz_off = cf_off[:, feet, 2]
    if not sc:                                   # control: no records; the crossed envs stand on their front feet
        assert np.abs(_substep(o, S0)[:, thighs]).max() == 0.0
        assert (fz_off[crossed].max(axis=1) > 10.0).all(), fz_off[crossed]
        print(f"[observed] oracle, self-collision off: front-foot f_z of the crossed envs {np.round(fz_off[crossed], 1).tolist()}")
        return
    cf = _substep(o, S0)
    f_l, f_r = cf[:, bn.index("LF_THIGH")], cf[:, bn.index("RF_THIGH")]
    pair = np.linalg.norm(f_l, axis=1)
    opposite = np.linalg.norm(f_l + f_r, axis=1) <= 0.02 * np.maximum(pair, 1e-9)
    fy = np.abs(cf[:, feet, 1])
    both = (fy > 50.0) & (fz_off > 10.0)         # a front foot pushed sideways by the other leg while the ground carries it
    print(f"[observed] oracle: thigh-pair force of the crossed envs {np.round(pair[crossed], 1).tolist()} N, front-foot |f_y| "
          f"{np.round(fy[crossed], 1).tolist()} N, the same feet's f_z without self-collision {np.round(fz_off[crossed], 1).tolist()} N, "
          f"largest thigh force of the other envs {np.abs(cf[~crossed][:, thighs]).max():.3g} N")
    assert ((pair > 50.0) & opposite)[crossed].any(), pair[crossed]
    assert both[crossed].any(), (fy[crossed], fz_off[crossed])
    assert np.abs(cf[~crossed][:, thighs]).max() == 0.0
    assert pair[N - 1] > 50.0 and opposite[N - 1] and both[N - 1].any()      # the partial workgroup's last env is one of them


def test_substep_with_self_collision_and_ground_contact_on_one_body(settled, oracle_without_self_collision):
    """k_physics<Anymal, plane, SC> (lg_physics_substep): one 5 ms sub-step from the crossed, standing state, every env."""
    sc, robot, p, o, d, fa, S_settled = settled
    S0 = _cross(d, S_settled, robot, p)
    _assert_inputs(sc, robot, o, oracle_without_self_collision, S0)
    cf_o = _substep(o, S0)
    qd0 = _np(S0["dof_state"]).reshape(N, 12, 2)[..., 1].astype(np.float64)
    _restore(d, S0)
    d.physics_substep(torch.zeros(N, 12), True)
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
    print(f"[observed] substep sc={sc}: velocity error / (1 + |dqd|) q99 {np.quantile(ratio, 0.99):.3g} max {ratio.max():.3g}, dof_pos {e_pos:.3g}, "
          f"root {e_root:.3g}, contact force {e_f:.3g} of {f_scale:.3g}")
    assert np.quantile(ratio, 0.99) <= 2e-4 and ratio.max() <= 1e-3, (float(np.quantile(ratio, 0.99)), float(ratio.max()))
    assert e_pos < 2e-5
    assert e_root < 1e-3
    assert e_f < 1e-3 * f_scale, (e_f, f_scale)
    assert np.array_equal(np.abs(cf_o).sum(axis=(1, 2)) > 1.0, np.abs(cf_d).sum(axis=(1, 2)) > 1.0)


def test_policy_kernels_with_self_collision_and_ground_contact_on_one_body(settled, oracle_without_self_collision):
    """lg_step, lg_step_policy and a 3-step lg_rollout_policy launch from the crossed, standing state, each step against the oracle."""
    sc, robot, p, o, d, fa, S_settled = settled
    S0 = _cross(d, S_settled, robot, p)
    _assert_inputs(sc, robot, o, oracle_without_self_collision, S0)
    obs0 = _np(S0["obs_buf"])
    report = {}
    # lg_step with fixed actions
    _restore(d, S0)
    act = (ACTION_SCALE * torch.randn(N, 12, generator=torch.Generator().manual_seed(2))).float()
    d.step(act.cuda(), C0)
    assert d.sim.device_status(True) == 0
    _check_oracle_step(o, S0, _snap(d), obs0, _np(d.buf["obs_buf"]), act.numpy(), _np(d.buf["rew_buf"]), _np(d.buf["reset_buf"]),
                       _np(d.buf["time_out_buf"]), C0, N, report)
    # lg_step_policy
    _restore(d, S0)
    actions, mean = d.step_policy(fa, d.buf["obs_buf"], C0)
    assert d.sim.device_status(True) == 0
    actions = _np(actions)
    _check_oracle_step(o, S0, _snap(d), obs0, _np(d.buf["obs_buf"]), actions, _np(d.buf["rew_buf"]), _np(d.buf["reset_buf"]),
                       _np(d.buf["time_out_buf"]), C0, N, report)
    # a 3-step lg_rollout_policy launch: S_k is the final state of a k-step launch from S_0 (_launch asserts device_status == 0)
    S = {0: S0}
    for k in range(1, STEPS + 1):
        st, S[k] = _launch(d, fa, S0, k, C0)
    roll = {k: _np(v) for k, v in st.items()}
    for t in range(STEPS):
        _check_oracle_step(o, S[t], S[t + 1], roll["obs"][t], roll["obs"][t + 1], roll["actions"][t], roll["rew"][t], roll["dones"][t],
                           roll["time_outs"][t], C0 + t, N, report)
    print(f"[observed] crossed and standing, sc={sc}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(report.items())))
