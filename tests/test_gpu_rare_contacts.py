"""-m gpu: the rarely-touching collision points of the quadruped (thigh, shank, base) in the fused policy kernels, against the oracle.

The rollout tests start from settled, standing robots: the thigh, shank and base points are off on every lane there, and the only
contacts the passes evaluate are the feet.  What the kernels do for a thigh, shank or base contact -- its record, its share of the
articulated-body passes, its exported force, the base row of contact_forces -- runs there for no lane, and never on a lane whose
neighbours in the wave have no such contact.  Here robots are PLACED so that some lanes of the rigid-body wave have such contacts and
most do not: anymal_c_flat, N = 20 -- one full workgroup of 16 envs and a partial one with 4 live envs, whose dead lanes replicate
env N - 1 -- with self-collision on and off.  That covers the mixed-lane rare contacts of every entry point in general, whatever a
kernel does wave-uniformly around them (the last pass's skipped corrector of the four-wave plane kernels is one such thing).

Poses (chosen on the CPU with the oracle; joint order LF, LH, RF, RH x HAA, HFE, KFE; the model has no joint position limits):
- KNEEL: knees bent the other way (front HFE 1.3, KFE 0.4; hind mirrored), base at z = 0.178: the knee ends of the four shank capsules
  are 2 mm in the ground, feet 25 mm and thighs 40 mm above it, 1 cm between the closest links; oracle: 200 - 700 N on every shank;
- TRUNK: legs folded above the trunk (HFE 2.3, KFE 1.2), base at z = 0.098: 2 mm of the base capsule in the ground; oracle: ~240 N on
  the base (and the env terminates);
- SIDE: rolled by 90 degrees onto the right side, right legs abducted by 0.6 rad so that the thigh shapes are lowest, z = 0.141: oracle:
  20 - 90 N on the RF and RH thighs.
Each case first asserts from the ORACLE's contact forces alone that these contacts exist (> 1 N on a shank, the base and a thigh
respectively; none of them in the standing case), then compares lg_step (fixed actions), lg_step_policy and every step of a 3-step
lg_rollout_policy launch with one oracle step from the same state and the kernel's actions: tests/test_gpu_rollout_oracle.py's
_check_oracle_step -- _compare_every_env with its TOLS, flags bit-equal, contact forces with the base row.  No env is set aside
beyond that helper's own rule.
"""
import numpy as np
import pytest
import torch

from tests.test_gpu_rollout_oracle import C0, _check_oracle_step, _flat_setup, _launch, _np, _restore, _snap, _state_to_oracle

pytestmark = pytest.mark.gpu

N = 20
STEPS = 3
_MIRROR = lambda hfe, kfe, haa_r=0.0: [0.0, hfe, kfe, 0.0, -hfe, -kfe, haa_r, hfe, kfe, haa_r, -hfe, -kfe]
#        joint positions                       base z  base quaternion (x, y, z, w)
KNEEL = (_MIRROR(1.3, 0.4),                    0.178, (0.0, 0.0, 0.0, 1.0))
TRUNK = (_MIRROR(2.3, 1.2),                    0.098, (0.0, 0.0, 0.0, 1.0))
SIDE = ([0.0, 0.4, -0.8, 0.0, -0.4, 0.8, 0.6, 0.4, -0.8, 0.6, -0.4, 0.8], 0.141, (0.70710678, 0.0, 0.0, 0.70710678))
CASES = {
    "standing": ({}, ()),                                            # no rare point touches
    "one_kneeling": ({5: KNEEL}, ("SHANK",)),                        # mixed lanes in the full workgroup
    "trunk_and_side": ({3: TRUNK, 9: SIDE}, ("base", "THIGH")),      # base point and thigh points on
    "last_env_kneeling": ({N - 1: KNEEL}, ("SHANK",)),               # its lanes are replicated onto the dead lanes of the partial workgroup
}


@pytest.fixture(scope="module", params=[True, False], ids=["sc_on", "sc_off"])
def settled(request):
    robot, p, o, d, ac, fa = _flat_setup(N, request.param)
    return robot, o, d, fa, _snap(d)


def _place(d, S, poses):
    """The settled state with the envs of ``poses`` re-posed at rest (their xy stays); they do not time out within the checked steps."""
    _restore(d, S)
    root, dof, ep = S["root_states"].clone(), S["dof_state"].clone().view(N, 12, 2), S["episode_length_buf"].clone()
    for e, (q, z, quat) in poses.items():
        root[e, 2] = z
        root[e, 3:7] = torch.tensor(quat, device=root.device)
        root[e, 7:] = 0.0
        dof[e, :, 0] = torch.tensor(q, device=dof.device)
        dof[e, :, 1] = 0.0
        ep[e] = 10
    d.buf["root_states"].copy_(root); d.buf["dof_state"].copy_(dof.view(S["dof_state"].shape)); d.buf["episode_length_buf"].copy_(ep)
    return _snap(d)


def _force_per_group(robot, cf):
    """Largest contact force (N) over the envs on a base / thigh / shank body."""
    f = np.linalg.norm(cf.astype(np.float64), axis=2)                 # (env, body)
    cols = lambda key: [i for i, n in enumerate(robot.body_names) if key in n]
    return {key: float(f[:, cols(key)].max()) for key in ("base", "THIGH", "SHANK")}


def _assert_contacts(robot, o, S0, actions, step, wanted):
    """From the oracle alone: the step from S0 loads the wanted bodies with more than 1 N -- and, standing, none of them."""
    _state_to_oracle(o, S0, _np(S0["obs_buf"]))
    o.step(actions, step)
    got = _force_per_group(robot, o.buf["contact_forces"])
    print(f"[observed] oracle contact forces, max over envs (N): {got}")
    for key in wanted:
        assert got[key] > 1.0, (key, got)
    if not wanted:
        assert max(got.values()) <= 1.0, got


@pytest.mark.parametrize("case", list(CASES))
def test_rare_contact_points_against_the_oracle(settled, case):
    robot, o, d, fa, S_settled = settled
    poses, wanted = CASES[case]
    S0 = _place(d, S_settled, poses)
    obs0 = _np(S0["obs_buf"])
    report = {}
    # lg_step with fixed actions
    act = (0.3 * torch.randn(N, 12, generator=torch.Generator().manual_seed(2))).float()
    _assert_contacts(robot, o, S0, act.numpy(), C0, wanted)
    d.step(act.cuda(), C0)
    assert d.sim.device_status(True) == 0
    _check_oracle_step(o, S0, _snap(d), obs0, _np(d.buf["obs_buf"]), act.numpy(), _np(d.buf["rew_buf"]), _np(d.buf["reset_buf"]),
                       _np(d.buf["time_out_buf"]), C0, N, report)
    # lg_step_policy
    _restore(d, S0)
    actions, mean = d.step_policy(fa, d.buf["obs_buf"], C0)
    assert d.sim.device_status(True) == 0
    actions = _np(actions)
    _assert_contacts(robot, o, S0, actions, C0, wanted)
    _check_oracle_step(o, S0, _snap(d), obs0, _np(d.buf["obs_buf"]), actions, _np(d.buf["rew_buf"]), _np(d.buf["reset_buf"]),
                       _np(d.buf["time_out_buf"]), C0, N, report)
    # a 3-step lg_rollout_policy launch: S_k is the final state of a k-step launch from S_0
    S = {0: S0}
    for k in range(1, STEPS + 1):
        st, S[k] = _launch(d, fa, S0, k, C0)
    roll = {k: _np(v) for k, v in st.items()}
    _assert_contacts(robot, o, S0, roll["actions"][0], C0, wanted)
    for t in range(STEPS):
        _check_oracle_step(o, S[t], S[t + 1], roll["obs"][t], roll["obs"][t + 1], roll["actions"][t], roll["rew"][t], roll["dones"][t],
                           roll["time_outs"][t], C0 + t, N, report)
    print(f"[observed] rare contacts {case}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(report.items())))
