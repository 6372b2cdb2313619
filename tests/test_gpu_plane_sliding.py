"""-m gpu: feet that leave the friction cone on the plane, in the fused policy kernels, against the oracle.

The rollout and rare-contact tests start from robots at rest: their feet stick, and the second articulated-body pass is entered with
the stick / secant impedance (bt > 0, fs = 0).  The other branch of the friction corrector -- a point whose predicted tangential
force exceeds mu f_n slides: constant force fs = -mu f_n vt / |vt|, bt = 0 -- runs for no lane there.  On the plane the contact
functions are written with the ground normal e_z taken out (csrc/lg_kernels.hip, "Plane builds"), and that branch is where their force
expression has the fewest terms in common with the general one.  Here some robots are PUSHED so that their feet slide while the
other envs of the wave stick: anymal_c_flat, N = 20 (one full workgroup of 16 envs and a partial one with 4 live envs, whose dead lanes
replicate env N - 1), self-collision on and off.

Inputs (chosen on the CPU with the oracle): from the settled state of tests/test_gpu_rollout_oracle._flat_setup, envs 2, 7, 12 and
N - 1 get a horizontal base velocity of 2 m/s in four different directions and friction_coeffs = 0, i.e. mu = 0.5 (0 + ground 1.0) / 2 =
0.5; every other env keeps its state and its friction (mu 0.7 - 1.2).  With the oracle's own settled state, eight action seeds and
action scales 0.3 and 1.0, the first step leaves 2 - 12 feet of the pushed envs on the cone and 15 - 29 feet of the others below half
of it, and no env resets within three steps.

Each entry point first asserts from the ORACLE's contact_forces alone that the case is what it claims: a foot of a pushed env carries
|f_t| within 2 % of mu f_n (the exported force of a sliding point is fs of the first pass next to f_n of the second, so the ratio is
not exactly 1), and a foot of another env carries less than half of mu f_n.  That is a condition on the inputs, not a tolerance of the
kernel.  Then lg_step (fixed actions), lg_step_policy and every step of a 3-step lg_rollout_policy launch are compared with one
oracle step from the same state and the kernel's actions: tests/test_gpu_rollout_oracle.py's _check_oracle_step with its TOLS.
"""
import numpy as np
import pytest
import torch

from tests.test_gpu_rollout_oracle import C0, _check_oracle_step, _flat_setup, _launch, _np, _restore, _snap, _state_to_oracle

pytestmark = pytest.mark.gpu

N = 20
STEPS = 3
PUSH = {2: (2.0, 0.0), 7: (0.0, -2.0), 12: (1.5, 1.5), N - 1: (-2.0, 0.5)}     # env: base velocity added (m/s, world x / y)
PUSH_FRICTION = 0.0


@pytest.fixture(scope="module", params=[True, False], ids=["sc_on", "sc_off"])
def settled(request):
    robot, p, o, d, ac, fa = _flat_setup(N, request.param)
    return robot, p, o, d, fa, _snap(d)


def _push(d, S):
    """The settled state with the envs of PUSH moving sideways on a slippery patch; they do not time out within the checked steps."""
    _restore(d, S)
    root, fr, ep = S["root_states"].clone(), S["friction_coeffs"].clone(), S["episode_length_buf"].clone()
    for e, (vx, vy) in PUSH.items():
        root[e, 7] += vx
        root[e, 8] += vy
        fr.view(-1)[e] = PUSH_FRICTION
        ep[e] = 10
    d.buf["root_states"].copy_(root); d.buf["friction_coeffs"].copy_(fr); d.buf["episode_length_buf"].copy_(ep)
    return _snap(d)


def _assert_sliding(robot, p, o, S0, actions, step):
    """From the oracle alone: the step from S0 leaves a foot of a pushed env on the friction cone and a foot of another env well inside."""
    _state_to_oracle(o, S0, _np(S0["obs_buf"]))
    o.step(actions, step)
    feet = [i for i, n in enumerate(robot.body_names) if "FOOT" in n]
    cf = o.buf["contact_forces"].reshape(N, -1, 3).astype(np.float64)[:, feet]
    mu = 0.5 * (o.buf["friction_coeffs"].reshape(N).astype(np.float64) + p.ground_friction)
    ft, fn = np.linalg.norm(cf[..., :2], axis=2), cf[..., 2]
    ratio = np.where(fn > 1.0, ft / np.maximum(mu[:, None] * fn, 1e-9), np.nan)         # feet that carry load
    pushed = np.zeros(N, bool)
    pushed[list(PUSH)] = True
    on_cone, inside = int((np.abs(ratio[pushed] - 1.0) <= 0.02).sum()), int((ratio[~pushed] < 0.5).sum())
    print(f"[observed] oracle: {on_cone} feet of the pushed envs on the cone (|f_t| / mu f_n: {np.round(ratio[pushed], 3).tolist()}), "
          f"{inside} feet of the other envs below half of it")
    assert on_cone >= 1 and inside >= 1, (on_cone, inside)
    assert int(pushed[-1]) == 1 and np.isfinite(ratio[-1]).any()                        # env N - 1 is one of them, with a loaded foot


def test_sliding_feet_against_the_oracle(settled):
    robot, p, o, d, fa, S_settled = settled
    S0 = _push(d, S_settled)
    obs0 = _np(S0["obs_buf"])
    report = {}
    # lg_step with fixed actions
    act = (0.3 * torch.randn(N, 12, generator=torch.Generator().manual_seed(2))).float()
    _assert_sliding(robot, p, o, S0, act.numpy(), C0)
    d.step(act.cuda(), C0)
    assert d.sim.device_status(True) == 0
    _check_oracle_step(o, S0, _snap(d), obs0, _np(d.buf["obs_buf"]), act.numpy(), _np(d.buf["rew_buf"]), _np(d.buf["reset_buf"]),
                       _np(d.buf["time_out_buf"]), C0, N, report)
    # lg_step_policy
    _restore(d, S0)
    actions, mean = d.step_policy(fa, d.buf["obs_buf"], C0)
    assert d.sim.device_status(True) == 0
    actions = _np(actions)
    _assert_sliding(robot, p, o, S0, actions, C0)
    _check_oracle_step(o, S0, _snap(d), obs0, _np(d.buf["obs_buf"]), actions, _np(d.buf["rew_buf"]), _np(d.buf["reset_buf"]),
                       _np(d.buf["time_out_buf"]), C0, N, report)
    # a 3-step lg_rollout_policy launch: S_k is the final state of a k-step launch from S_0
    S = {0: S0}
    for k in range(1, STEPS + 1):
        st, S[k] = _launch(d, fa, S0, k, C0)
    roll = {k: _np(v) for k, v in st.items()}
    _assert_sliding(robot, p, o, S0, roll["actions"][0], C0)
    for t in range(STEPS):
        _check_oracle_step(o, S[t], S[t + 1], roll["obs"][t], roll["obs"][t + 1], roll["actions"][t], roll["rew"][t], roll["dones"][t],
                           roll["time_outs"][t], C0 + t, N, report)
    print(f"[observed] plane sliding: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(report.items())))
