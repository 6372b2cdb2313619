"""-m gpu: the branches of the contact evaluation and of the speed-limit terms in the articulated-body passes, each driven on
purpose, against the oracle.

contact_evaluate (csrc/lg_kernels.hip) decides per contact point and pass: still in contact or leaving (fn <= 0), beyond the friction
cone (slide with mu fn against the predicted slip) or inside it (re-aim the secant; a point with bt = 0 keeps it), and a point no
lane of the wave has in contact is skipped as a whole.  The settled parity states stand still on four sticking feet, so no other
test takes the leaving, the sliding or the bt = 0 side on purpose, or has a thigh / shank point in contact on a single lane.

N = 20: one full workgroup of 16 envs and a partial one with 4 live envs, whose dead lanes replicate env N - 1.  Every case sits in
env FIRST (first workgroup) and in env N - 1; every other env keeps the settled state (CONTROL is one of them) and is compared too.
The state is the one tests/test_gpu_rollout_oracle._flat_setup settles (anymal_c_flat, self-collision on, and off); the torques are
the ones that state stands on (its `torques` buffer) unless a case says otherwise.

Each case first asserts from the ORACLE alone that its inputs enter the branch it names (conditions on inputs, not tolerances of the
kernel).  [observed] figures: the oracle's own settled state (8 zero-action steps from the reset), self-collision on.
(a) leaving.  Root velocity +0.6 m/s upwards: every foot is inside the margin at set-up (the unedited twin run loads it) and
    kn v_z outweighs K depth in pass 0: the oracle's force on all four feet is exactly 0.  [observed] twin 146 - 292 N per foot.
(b) stick -> slide.  friction_coeffs = 0 (mu = (0 + ground_friction) / 2 = 0.5, the smallest the engine has) and +20 N m on the four
    HFE drives: the hind feet need more than mu fn to stick.  Slid, the tangential force of pass 1 is the constant mu fn of PASS 0 while
    the reported normal force is pass 1's, so |ft| / (mu fn) is 1 up to the change of fn between the passes: asserted within
    [0.8, 1.25]; and with mu doubled (friction_coeffs = 1) the same foot sticks with a force more than 15 % larger.
    [observed] LH foot |ft| / (mu fn) 1.115 / 1.110, |ft| 167 / 141 N against 223 / 181 N with mu doubled.
(c) inside the cone.  Re-aim: +0.02 m/s of slip, every loaded foot keeps 0 < |ft| < mu fn ([observed] 0.45 - 0.60 mu fn).  First touch
    with bt = 0: the state's previous contact forces zeroed (the secant's seed) and 0.1 m/s of slip: bt starts at 0 and stays there,
    the feet are loaded (fn > 0) and their tangential force is exactly 0.  [observed] fn 99 - 195 N.
(d) the wave-uniform skip, both ways.  One lane with a shank contact: the case env's base 0.1 m lower, its LF leg at HFE 0 / KFE 1.25 rad,
    the LF shank carries load ([observed] 2612 / 1768 N) and no thigh, shank or base point of any other env does.  And no lane with any:
    all 16 envs of the first workgroup lifted by 5 mm, less than the contact margin, feet loaded, nothing else ([observed] feet
    0 - 238 N, at least two of an env's loaded, against 0 - 292 N unlifted).
(e) speed-limit damper armed in pass 0 on one lane of the wave: case (b) of tests/test_gpu_joint_terms.py, lifted, zero torques but
    -80 N m on LF_KFE at -10 rad/s.
(f) control: env CONTROL (17 where the whole first workgroup is the case) is untouched in every case.

Then lg_physics_substep (k_physics<Anymal, plane, SC / !SC>) against the oracle's physics_substep, every env, with the bounds of
tests/test_gpu_compact_inertia.test_substep_with_self_collision_and_ground_contact_on_one_body (through
tests/test_gpu_joint_terms._check_substep).  Nothing new is bounded.

The tests pin behaviour, not an implementation: they pass on the library of the commit before the select form as well.
"""
import numpy as np
import pytest

from tests.test_gpu_joint_terms import (CONTROL, FIRST, N, _check_substep, _oracle_substep, _oracle_without_speed_limit, _untouched,
                                        _with_dof)
from tests.test_gpu_rollout_oracle import _flat_setup, _np, _snap

pytestmark = pytest.mark.gpu

ENVS = (FIRST, N - 1)
CONTROL_2 = 17                       # second workgroup


@pytest.fixture(scope="module", params=[True, False], ids=["sc_on", "sc_off"])
def anymal(request):
    sc = request.param
    robot, p, o, d, ac, fa = _flat_setup(N, sc)
    S = _snap(d)
    names = list(robot.body_names)
    feet = [i for i, n in enumerate(names) if n.endswith("_FOOT")]
    rest = [i for i in range(len(names)) if i not in feet]
    assert len(feet) == 4 and names[feet[1]] == "LH_FOOT"
    kfe, hfe = list(robot.dof_names).index("LF_KFE"), list(robot.dof_names).index("LF_HFE")
    o_free = _oracle_without_speed_limit("anymal_c_flat", kfe, tweak=lambda c: setattr(c.asset, "self_collisions", 0 if sc else 1))
    return dict(sc=sc, p=p, o=o, d=d, S=S, tau=_np(S["torques"]).reshape(N, 12).astype(np.float32).copy(), feet=feet, rest=rest,
                shank=names.index("LF_SHANK"), hfes=[i for i, n in enumerate(robot.dof_names) if n.endswith("_HFE")], kfe=kfe, hfe=hfe,
                o_free=o_free, vlim=float(o.model.dof_vel_limit[kfe]))


def _edited(S, edit):
    S0 = {k: v.clone() for k, v in S.items()}
    edit(S0)
    return S0


def _mu(A, S0, e):
    return 0.5 * (float(S0["friction_coeffs"].reshape(-1)[e]) + float(A["p"].ground_friction))


def test_foot_leaves_contact_in_the_first_pass(anymal):
    """(a): in contact at set-up, fn <= 0 in pass 0."""
    A = anymal
    o, feet = A["o"], A["feet"]

    def up(S0):
        for e in ENVS:
            S0["root_states"][e, 9] = 0.6
    S0 = _edited(A["S"], up)
    _, cf_twin = _oracle_substep(o, A["S"], A["tau"])
    _, cf = _oracle_substep(o, S0, A["tau"])
    print(f"[observed] oracle, leaving sc={A['sc']}: twin foot fn {cf_twin[list(ENVS)][:, feet, 2].tolist()}")
    for e in ENVS:
        assert (cf_twin[e, feet, 2] > 0.0).all()
        assert (cf[e] == 0.0).all()
    assert _untouched(A["S"], S0, CONTROL)
    _check_substep(o, A["d"], S0, A["tau"], f"leaving sc={A['sc']}")


def test_sticking_foot_starts_to_slide(anymal):
    """(b): bt vtm > mu fn after pass 0, the LH foot."""
    A = anymal
    o, f = A["o"], A["feet"][1]
    tau = A["tau"].copy()
    for e in ENVS:
        tau[e, A["hfes"]] += 20.0

    def friction(c):
        def edit(S0):
            for e in ENVS:
                S0["friction_coeffs"].reshape(-1)[e] = c
        return edit
    S0, S_2mu = _edited(A["S"], friction(0.0)), _edited(A["S"], friction(1.0))
    _, cf_2mu = _oracle_substep(o, S_2mu, tau)
    _, cf = _oracle_substep(o, S0, tau)
    for e in ENVS:
        mu = _mu(A, S0, e)
        assert _mu(A, S_2mu, e) == 2.0 * mu
        ft, ft_2mu, fn = np.hypot(cf[e, f, 0], cf[e, f, 1]), np.hypot(cf_2mu[e, f, 0], cf_2mu[e, f, 1]), cf[e, f, 2]
        print(f"[observed] oracle, slide sc={A['sc']} env {e}: |ft| {ft:.4g} = {ft / (mu * fn):.4g} mu fn, {ft_2mu:.4g} with mu doubled")
        assert fn > 0.0 and 0.8 <= ft / (mu * fn) <= 1.25
        assert ft_2mu > 1.15 * ft
    assert _untouched(A["S"], S0, CONTROL)
    _check_substep(o, A["d"], S0, tau, f"slide sc={A['sc']}")


def test_slipping_foot_inside_the_cone_is_reaimed(anymal):
    """(c): bt > 0, bt vtm <= mu fn."""
    A = anymal
    o, feet = A["o"], A["feet"]

    def slip(S0):
        for e in ENVS:
            S0["root_states"][e, 7] += 0.02
    S0 = _edited(A["S"], slip)
    _, cf = _oracle_substep(o, S0, A["tau"])
    for e in ENVS:
        ft, fn = np.hypot(cf[e, feet, 0], cf[e, feet, 1]), cf[e, feet, 2]
        on = fn > 0.0
        print(f"[observed] oracle, re-aim sc={A['sc']} env {e}: |ft| / (mu fn) {(ft[on] / (_mu(A, S0, e) * fn[on])).tolist()}")
        assert on.sum() >= 2 and (ft[on] > 0.0).all() and (ft[on] < _mu(A, S0, e) * fn[on]).all()
    assert _untouched(A["S"], S0, CONTROL)
    _check_substep(o, A["d"], S0, A["tau"], f"re-aim sc={A['sc']}")


def test_first_touch_without_a_previous_force_keeps_zero_friction(anymal):
    """(c): bt = 0 at set-up stays 0 -- no tangential force in this sub-step."""
    A = anymal
    o, feet = A["o"], A["feet"]

    def touch(S0):
        for e in ENVS:
            S0["root_states"][e, 7] = 0.1
            S0["contact_forces"].reshape(N, -1, 3)[e] = 0.0
    S0 = _edited(A["S"], touch)
    _, cf = _oracle_substep(o, S0, A["tau"])
    print(f"[observed] oracle, first touch sc={A['sc']}: fn {cf[list(ENVS)][:, feet, 2].tolist()}")
    for e in ENVS:
        assert (cf[e, feet, 2] > 0.0).sum() >= 2
        assert (cf[e, :, :2] == 0.0).all()
    assert _untouched(A["S"], S0, CONTROL)
    _check_substep(o, A["d"], S0, A["tau"], f"first touch sc={A['sc']}")


def test_one_lane_of_the_wave_with_a_shank_contact(anymal):
    """(d): the per-point skip entered for a point that a single lane has in contact."""
    A = anymal
    o, rest, shank = A["o"], A["rest"], A["shank"]

    def kneel(S0):
        for e in ENVS:
            S0["root_states"][e, 2] -= 0.1
    S0 = _with_dof(A["d"], _edited(A["S"], kneel), [(e, A["hfe"], 0, 0.0) for e in ENVS] + [(e, A["kfe"], 0, 1.25) for e in ENVS])
    _, cf = _oracle_substep(o, S0, A["tau"])
    print(f"[observed] oracle, shank contact sc={A['sc']}: LF_SHANK fn {cf[list(ENVS), shank, 2].tolist()}")
    loaded = np.zeros((N, cf.shape[1]), bool)
    for e in ENVS:
        loaded[e, shank] = True
        assert cf[e, shank, 2] > 100.0
    assert not np.abs(cf[:, rest])[~loaded[:, rest]].any()                # no other thigh / shank / base point of any env
    assert _untouched(A["S"], S0, CONTROL)
    _check_substep(o, A["d"], S0, A["tau"], f"shank contact sc={A['sc']}")


def test_first_workgroup_lifted_inside_the_foot_margin(anymal):
    """(d): the per-point skip taken for every thigh, shank and base point of a wave whose feet are all inside the margin."""
    A = anymal
    o, feet, rest = A["o"], A["feet"], A["rest"]
    lift = 0.005
    assert lift < float(A["p"].contact_margin)

    def up(S0):
        S0["root_states"][:16, 2] += lift
    S0 = _edited(A["S"], up)
    _, cf_twin = _oracle_substep(o, A["S"], A["tau"])
    _, cf = _oracle_substep(o, S0, A["tau"])
    print(f"[observed] oracle, lifted workgroup sc={A['sc']}: foot fn {cf[:16][:, feet, 2].min():.4g} - {cf[:16][:, feet, 2].max():.4g}")
    assert not np.abs(cf[:16][:, rest]).any()
    assert ((cf[:16][:, feet, 2] > 0.0).sum(axis=1) >= 2).all() and (cf[:16][:, feet, 2] != cf_twin[:16][:, feet, 2]).any(axis=1).all()
    assert _untouched(A["S"], S0, CONTROL_2)
    _check_substep(o, A["d"], S0, A["tau"], f"lifted workgroup sc={A['sc']}")


def test_speed_limit_damper_armed_on_one_lane(anymal):
    """(e): one lane of each wave arms the damper in pass 0; the parent joint feels its reaction in pass 1."""
    A = anymal
    o, d, j, hfe, vlim = A["o"], A["d"], A["kfe"], A["hfe"], A["vlim"]

    def up(S0):
        for e in ENVS:
            S0["root_states"][e, 2] += 0.05
    S0 = _with_dof(d, _edited(A["S"], up), [(e, j, 1, -10.0) for e in ENVS])
    tau = np.zeros((N, 12), np.float32)
    for e in ENVS:
        tau[e, j] = -80.0
    qd_free, _ = _oracle_substep(A["o_free"], S0, tau)
    qd_new, _ = _oracle_substep(o, S0, tau)
    print(f"[observed] oracle, damper sc={A['sc']}: qd' {qd_new[list(ENVS), j].tolist()}, LF_HFE {qd_new[list(ENVS), hfe].tolist()} against "
          f"{qd_free[list(ENVS), hfe].tolist()} without the limit")
    for e in ENVS:
        assert abs(qd_new[e, j]) == vlim
        assert qd_new[e, hfe] != qd_free[e, hfe] and abs(qd_free[e, j]) > vlim
    others = [e for e in range(N) if e not in ENVS]
    assert (np.abs(qd_new[others]) < vlim).all()                       # no other lane of either wave is on a limit
    assert _untouched(A["S"], S0, CONTROL)
    qd_dev = _check_substep(o, d, S0, tau, f"damper sc={A['sc']}")
    for e in ENVS:
        assert abs(qd_dev[e, j]) == vlim
