"""CPU, oracle only: the references and the inputs of the height-field contact tests (tests/hf_cases.py), proved before any kernel is
involved.  tests/test_gpu_hf_contact.py runs the same cases on the device.

a. test_oracle_force_direction: the oracle's ground_contact against the float64 restatement ground_contact64, read through the
   frictionless force direction of single-sphere feet, on ramps, twisted cells, faces and edges in all four directions, corner cells
   and the four map edges.
b. test_oracle_rotation_equivalence: a robot on an exact ramp under gravity (0, 0, -g) against the same robot on the plane build under
   gravity R^T (0, 0, -g).
c. test_*_inputs: every case is what it claims, from the oracle and ground_contact64 alone, with guard bands around every decision.
"""
import collections
import functools

import numpy as np
import pytest

from tests import hf_cases as H
from oracle.oracle import OracleSim

N = H.N


def _state(o):
    return o.buf["root_states"].copy(), o.buf["dof_state"].copy(), o.buf["contact_forces"].copy()


# ------------------------------------------------------------------ a. frictionless force direction
@functools.lru_cache(maxsize=None)
def direction_case(task, kind):
    """The designed standing state on field ``kind``, the oracle's frictionless sub-step from it and ground_contact64 of every sphere."""
    terr, cfg, robot, p, model, w = H.field_setup(task, kind)
    S = terr.heightsamples
    root, q, notes = H.standing_states(robot, p, S, kind, seed=1)
    o = OracleSim(p, model, robot, w, threads=8)
    o.set_terrain(S, terr.env_origins)
    H.load_state(o, root, np.stack((q, np.zeros_like(q)), 2), np.full(N, -float(p.ground_friction)))
    root32, q32 = o.buf["root_states"].astype(np.float64), o.dof_pos.astype(np.float64)      # what the engine reads
    o.physics_substep(np.zeros((N, 12), np.float32), True)
    after = _state(o)
    cf = o.buf["contact_forces"].astype(np.float64).reshape(N, -1, 3)
    o.physics_substep(np.zeros((N, 12), np.float32), True)
    contacts = [H.contacts64(robot, p, S, root32[e], q32[e]) for e in range(N)]
    return dict(robot=robot, p=p, model=model, w=w, terr=terr, samples=S, notes=notes, root=root32, q=q32, cf=cf, contacts=contacts,
                friction=np.full(N, -float(p.ground_friction)), trace=[after, _state(o)])


def check_force_direction(robot, p, contacts, cf, label):
    """Every loaded single-sphere body reports f / |f| = n64 (bounds: H.DIRECTION_BOUND per branch); a single-sphere body whose float64
    depth is below -contact_margin - 1e-5 reports exactly 0.  Returns the worst deviation per branch class ('smooth', 'edge')."""
    worst, loaded = {"smooth": 0.0, "edge": 0.0}, 0
    for e in range(len(contacts)):
        per = collections.defaultdict(list)
        for b, res in contacts[e]:
            per[b].append(res)
        for b, rs in per.items():
            if len(rs) != 1:
                continue
            f = cf[e, b]
            nf = float(np.linalg.norm(f))
            if rs[0]["depth"] < -float(p.contact_margin) - 1e-5:
                assert nf == 0.0, (label, e, robot.body_names[b], f)
            if nf > 1.0:
                cls = "edge" if rs[0]["branch"].endswith("edge") else "smooth"
                worst[cls] = max(worst[cls], float(np.abs(f / nf - rs[0]["n"]).max()))
                loaded += 1
    print(f"[observed] {label}: max |f/|f| - n64| smooth {worst['smooth']:.3g} edge {worst['edge']:.3g} over {loaded} loaded single-sphere bodies")
    for cls in worst:
        assert worst[cls] <= H.DIRECTION_BOUND[cls], (label, cls, worst[cls])
    return worst, loaded


@pytest.mark.parametrize("task,kind", [("anymal_c_rough", k) for k in H.DIRECTION_FIELDS] + [("a1", k) for k in ("ramp_b", "twist", "edge")])
def test_oracle_force_direction(oracle_lib, task, kind):
    """With friction_coeffs = -ground_friction the combined friction is 0 and the exported force of a single-sphere foot is f_n n: its
    direction is the contact normal the engine used.  Against ground_contact64 at the float64 value of the fp32 state.
    [observed] worst over all cases, contacts with the ground patch or a face ('smooth'; a face normal is exact): 1.1e-6, a few fp32 ulp
    of a unit vector -> bound 4 x = 4.4e-6.  Contacts with a face's top EDGE: 5.4e-5 -> bound 2.2e-4.  The edge normal is (dist, dz) /
    len with len within the 3 cm foot radius and dist = (grid coordinate - its floor) x 0.1 m, where the fp32 grid coordinate near 160
    carries 1.5e-5 cells = 1.5e-6 m of rounding: 1.5e-6 / 0.03 = 5e-5 of direction, which is what is seen; it is rounding of the
    sphere position, not of the rule (the same feet on a face or on the ground agree to 1e-6)."""
    c = direction_case(task, kind)
    worst, loaded = check_force_direction(c["robot"], c["p"], c["contacts"], c["cf"], f"oracle {task} {kind}")
    assert loaded >= 40, loaded


# ------------------------------------------------------------------ b. rotation equivalence
@functools.lru_cache(maxsize=None)
def rotation_case(task, case):
    """Both worlds of a rotation-equivalence case, the oracle pair's chained sub-steps and its per-step env masks."""
    kind = H.ROT_RAMP[case]
    slope, sc = H.RAMP_SLOPES[kind], case == "crossed"
    terr, cfg, robot, p, model, w = H.field_setup(task, kind, sc=sc)
    R = H.rotation_from_normal(H.ramp_normal(slope))
    cfg_p, robot_p, p_p, model_p, w_p = H.plane_setup(task, R.T @ np.array([0.0, 0.0, -H.G]), sc=sc)
    o_r = OracleSim(p, model, robot, w, threads=8)
    o_r.set_terrain(terr.heightsamples, terr.env_origins)
    o_p = OracleSim(p_p, model_p, robot_p, w_p, threads=8)
    desc = H.body_description(task, robot, p, case, seed=H.ROT_SEED.get((task, case), 1))
    plane, ramp, dof, R, anchor = H.paired_states(robot, p, slope, desc)
    H.assert_inside_map(robot, p, ramp, desc["q"])
    H.load_state(o_r, ramp, dof, desc["friction"])
    H.load_state(o_p, plane, dof, desc["friction"])
    tau = desc["tau"].astype(np.float32)
    trace = []                                                                     # oracle states after every sub-step, both worlds

    def sub(o):
        def f(t, wc):
            o.physics_substep(t, wc)
            trace.append(_state(o))
        return f
    worst, masks, errs = H.run_rotation_pair(sub(o_r), sub(o_p), lambda: _state(o_r), lambda: _state(o_p), tau, R, anchor)
    return dict(task=task, case=case, kind=kind, sc=sc, terr=terr, robot=robot, p=p, model=model, w=w, p_plane=p_p, model_plane=model_p, w_plane=w_p, desc=desc,
                plane=plane, ramp=ramp, dof=dof, tau=tau, R=R, anchor=anchor, worst=worst, masks=masks, errs=errs,
                ramp_trace=trace[0::2], plane_trace=trace[1::2])


@pytest.mark.parametrize("task,case", H.ROT_TASK_CASES)
def test_oracle_rotation_equivalence(oracle_lib, task, case):
    """Six chained sub-steps, compared from the second on, forces / velocities / positions of the ramp world rotated back, joint states
    directly; an env is compared while both oracle runs report the same set of loaded bodies (at most 5 % may drop out: one env of one case does).
    [observed] worst over the compared envs (force: share of the largest force of the sub-step; root_vel: m/s and rad/s; dof_vel: rad/s):
      anymal_c_rough  stick (ramp_a)        force 7.7e-05  root_vel 6.7e-06  root_pos 1.8e-06  dof_pos 1.7e-06  dof_vel 1.1e-04
      anymal_c_rough  slide (ramp_b)        force 4.5e-05  root_vel 9.2e-06  root_pos 1.5e-06  dof_pos 1.2e-06  dof_vel 1.1e-04
      anymal_c_rough  frictionless (ramp_c) force 1.4e-05  root_vel 3.6e-06  root_pos 2.2e-06  dof_pos 1.7e-06  dof_vel 1.1e-04
      anymal_c_rough  crossed (ramp_b)      force 9.0e-05  root_vel 4.8e-05  root_pos 2.2e-06  dof_pos 2.4e-06  dof_vel 1.8e-04
      a1              stick                 force 1.5e-05  root_vel 6.3e-05  root_pos 1.8e-06  dof_pos 6.1e-07  dof_vel 7.0e-05
      a1              slide                 force 2.7e-05  root_vel 2.0e-04  root_pos 1.7e-06  dof_pos 3.2e-06  dof_vel 3.6e-04
      a1              frictionless          force 3.2e-05  root_vel 2.6e-05  root_pos 2.0e-06  dof_pos 1.3e-06  dof_vel 1.1e-04   (1 env dropped)
      a1              crossed               force 3.4e-05  root_vel 3.8e-04  root_pos 1.7e-06  dof_pos 8.4e-06  dof_vel 4.4e-04
      cassie          stick                 force 1.2e-04  root_vel 2.7e-05  root_pos 2.0e-06  dof_pos 8.9e-06  dof_vel 3.9e-04
      cassie          slide                 force 1.6e-04  root_vel 2.5e-05  root_pos 2.0e-06  dof_pos 9.9e-06  dof_vel 6.2e-04
      cassie          frictionless          force 8.5e-05  root_vel 3.0e-06  root_pos 2.0e-06  dof_pos 1.4e-05  dof_vel 7.1e-04
    (Cassie standing still uses seed 2, see H.ROT_SEED: with seed 1 one toe of one env takes another branch in the two worlds, force 1.6e-2.)
    H.ROT_OBSERVED holds the worst per robot, rounded up; the device test's bounds are 4 x those.  A wrong term of the general-normal
    text (tangential projection, r x n, sliding force) moves these figures by orders of magnitude."""
    c = rotation_case(task, case)
    dropped = int((~c["masks"][-1]).sum())
    print(f"[observed] oracle pair {task} {case}: " + ", ".join(f"{k} {v:.3g}" for k, v in c["worst"].items()) + f", envs dropped {dropped} of {N}")
    assert dropped <= 0.05 * N, dropped
    for k, v in c["worst"].items():
        assert v <= H.ROT_OBSERVED[task][k], (k, v)


# ------------------------------------------------------------------ c. input conditions
def _guard_bands(c, cells):
    """No sphere within 1e-5 m of the contact on / off threshold, no candidate tie within 1e-5 m, and (riser cases) no sphere centre within
    1e-4 cells of a cell boundary."""
    margin = float(c["p"].contact_margin)
    for e in range(N):
        for b, res in c["contacts"][e]:
            assert abs(res["depth"] + margin) > 1e-5, (e, b, res["depth"])
            d = sorted(res["cand"].values())
            assert all(d[i + 1] - d[i] > 1e-5 for i in range(len(d) - 1)) or res["depth"] < -margin - 1e-3, (e, b, res["cand"])
            if cells:
                assert ((res["t"] > 1e-4) & (res["t"] < 1 - 1e-4)).all(), (e, b, res["t"])


def _loaded_single(c, e):
    """[(report body, result)] of env e's loaded single-sphere bodies."""
    per = collections.defaultdict(list)
    for b, res in c["contacts"][e]:
        per[b].append(res)
    return [(b, rs[0]) for b, rs in per.items() if len(rs) == 1 and np.linalg.norm(c["cf"][e, b]) > 1.0]


@pytest.mark.parametrize("kind", ["ramp_a", "ramp_b", "ramp_c", "twist"])
def test_ramp_and_twist_inputs(oracle_lib, kind):
    """Feet loaded on the slope in every env (env N - 1 included), every collision point at least 0.5 m inside the map; the ramps' normal is
    the designed one, the twisted patch's cells are not planar and its normal differs between the loaded feet of one robot."""
    c = direction_case("anymal_c_rough", kind)
    H.assert_inside_map(c["robot"], c["p"], c["root"], c["q"])
    _guard_bands(c, cells=False)
    loaded = [_loaded_single(c, e) for e in range(N)]
    assert all(len(l) >= 1 for l in loaded) and len(loaded[N - 1]) >= 1
    if kind != "twist":
        n = H.ramp_normal(H.RAMP_SLOPES[kind])
        assert abs(n[2] - 1.0) > 0.01
        assert max(np.abs(r["n"] - n).max() for l in loaded for b, r in l) < 1e-7           # float64 of the fp32 scales: 0.005f / 0.1f
        assert sum(len(l) for l in loaded) >= 3 * N
    else:
        S = c["samples"].astype(np.int64)
        twist = [abs(S[r["cell"][0], r["cell"][1]] + S[r["cell"][0] + 1, r["cell"][1] + 1] - S[r["cell"][0] + 1, r["cell"][1]] - S[r["cell"][0], r["cell"][1] + 1])
                 for l in loaded for b, r in l]
        assert (np.array(twist) > 0).all()                                                 # every loaded foot stands in a non-planar cell
        spread = [max(np.abs(r["n"] - l[0][1]["n"]).max() for b, r in l) for l in loaded if len(l) >= 2]
        assert len(spread) >= 5 and max(spread) > 0.02
        assert max(1.0 - r["n"][2] for l in loaded for b, r in l) > 0.01


def test_plateau_inputs(oracle_lib):
    """The riser cases take the branch they were designed for, decided by which candidate ground_contact64 reports as deepest: loaded feet on
    faces and on top edges with normals towards -x, +x, -y and +y, feet in outer corner cells on the face and on its sloping top edge, a
    foot in the inner corner cell with both candidates present and either one deeper; env N - 1 stands in an outer corner cell."""
    c = direction_case("anymal_c_rough", "plateau")
    _guard_bands(c, cells=True)
    seen = collections.Counter()
    for e in range(N):
        kind, branch = c["notes"][e]
        for b, r in _loaded_single(c, e):
            if r["branch"] != "ground":
                ax = "xy".index(r["branch"][0])
                seen[(r["branch"], "+" if r["n"][ax] > 0 else "-")] += 1
                if len([k for k in r["cand"] if k != "ground"]) == 2:
                    seen[("both axes", r["branch"])] += 1
                S = c["samples"]
                high = sum(int(S[r["cell"][0] + a, r["cell"][1] + d] > 0) for a in (0, 1) for d in (0, 1))
                if high == 1:
                    seen[("outer corner", r["branch"])] += 1
    print("[observed] plateau: loaded single-sphere feet per deepest branch and normal sign", dict(seen))
    for br in ("x-face", "x-edge", "y-face", "y-edge"):
        for sign in "+-":
            assert seen[(br, sign)] >= 2, (br, sign, seen)
    assert seen[("outer corner", "x-face")] >= 4 and seen[("outer corner", "x-edge")] >= 2
    assert seen[("both axes", "x-face")] >= 1 and seen[("both axes", "y-face")] >= 1
    assert c["notes"][N - 1][0].startswith("corner") and any(r["branch"] != "ground" for b, r in _loaded_single(c, N - 1))


def test_map_edge_inputs(oracle_lib):
    """The edge rows / columns hold non-zero, sloping samples; on each of the four sides an env stands with a loaded foot on the map and a
    loaded foot beyond it; env N - 1 stands beyond the corner with every collision point at negative grid coordinates, loaded."""
    c = direction_case("anymal_c_rough", "edge")
    _guard_bands(c, cells=False)
    S = c["samples"].astype(np.int64)
    for line in (S[0], S[-1], S[:, 0], S[:, -1]):
        assert (line != 0).all() and np.abs(np.diff(line)).max() >= 1 and len(np.unique(line)) > 50
    rows, cols = S.shape
    astride = collections.Counter()
    for e in range(N):
        g = [(r["cell"], b) for b, r in _loaded_single(c, e)]
        beyond = {"x-lo": [cell[0] < 0 for cell, b in g], "x-hi": [cell[0] >= rows - 1 for cell, b in g],
                  "y-lo": [cell[1] < 0 for cell, b in g], "y-hi": [cell[1] >= cols - 1 for cell, b in g]}
        for side, flags in beyond.items():
            if any(flags) and not all(flags):
                astride[side] += 1
    print("[observed] map edge: envs with loaded feet on both sides of the edge", dict(astride))
    for side in ("x-lo", "x-hi", "y-lo", "y-hi"):
        assert astride[side] >= 2, astride
    assert all(r["cell"][0] < 0 and r["cell"][1] < 0 for b, r in c["contacts"][N - 1]) and len(_loaded_single(c, N - 1)) >= 2


@pytest.mark.parametrize("task,case", H.ROT_TASK_CASES)
def test_rotation_case_inputs(oracle_lib, task, case):
    """From the oracle pair alone: at every compared sub-step more than half of the envs carry load on the slope (the robots are dropped
    0.5 - 4 mm into a 1e6 N/m ground and some feet lift again), env N - 1 does at one of them; 'slide': the pushed envs (three in four, env N - 1 one of them)
    still move at more than 1 m/s along the surface after the last sub-step while the others stay below 0.5 m/s, and at one of the compared
    sub-steps at least 20 loaded bodies of the pushed envs sit within 5 % of the friction cone at mu_bar = 0.5 (median |f_t| / mu f_n above 0.85); 'stick': at mu_bar = 1 no
    base moves faster than 0.15 m/s along the surface and the median loaded body is inside half of the cone; 'frictionless': no tangential force at all; 'crossed': in the first sub-step a crossed env
    (every third, env N - 1 among them) carries a self-collision force of more than 50 N (A1: 0.5 N) and a ground force of more than 10 N (A1: 1 N)
    along the normal on the SAME leaf body (shank and foot are one rigid body), and no other env carries a self-collision force."""
    c = rotation_case(task, case)
    robot, p = c["robot"], c["p"]
    assert all(err["loaded"].any(axis=1).mean() > 0.5 for err in c["errs"]) and any(err["loaded"][N - 1].any() for err in c["errs"])
    mu = 0.5 * (c["desc"]["friction"] + float(p.ground_friction))

    def cone_ratio(step):
        """|f_t| / (mu f_n) of every loaded body after sub-step `step` (plane frame: the normal is e_z).  The exported force of a sliding
        point is the sliding force of the first pass next to f_n of the second, so the ratio of a sliding foot is near 1, not exactly 1."""
        cf = c["plane_trace"][step][2].astype(np.float64).reshape(N, -1, 3)
        ft, fn = np.linalg.norm(cf[..., :2], axis=2), cf[..., 2]
        return np.where(fn > 1.0, ft / np.maximum(mu[:, None] * fn, 1e-9), np.nan)
    speed = np.linalg.norm(c["plane_trace"][-1][0][:, 7:9].astype(np.float64), axis=1)        # base speed along the surface, last sub-step
    last = cone_ratio(H.ROT_STEPS - 1)
    if case == "slide":
        moving = np.linalg.norm(c["desc"]["v"][:, :2], axis=1) > 1.0
        med = float(np.nanmedian(last[moving]))
        n1 = np.concatenate([cone_ratio(s)[N - 1] for s in range(1, H.ROT_STEPS)])
        print(f"[observed] {task} slide: median |f_t| / mu f_n over {int(np.isfinite(last[moving]).sum())} loaded bodies of the pushed envs {med:.3f}, "
              f"env N - 1 {np.round(n1[np.isfinite(n1)], 2).tolist()}, base speed pushed {speed[moving].min():.2f} - {speed[moving].max():.2f} m/s, others < {speed[~moving].max():.2f}")
        assert moving[N - 1] and moving.sum() >= 25 and (~moving).sum() >= 5
        assert (speed[moving] > 1.0).all() and (speed[~moving] < 0.5).all()          # the pushed envs keep sliding, the others do not start
        assert np.isfinite(last[moving]).sum() >= 20
        per_step = [cone_ratio(s)[moving] for s in range(1, H.ROT_STEPS)]
        on_cone = [int((np.abs(r - 1.0) <= 0.05).sum()) for r in per_step]
        best = int(np.argmax(on_cone))
        print(f"[observed] {task} slide: loaded bodies of the pushed envs within 5 % of the cone, sub-steps 2 - {H.ROT_STEPS}: {on_cone}, median at the best {np.nanmedian(per_step[best]):.3f}")
        assert on_cone[best] >= 20 and np.nanmedian(per_step[best]) >= 0.85
        assert np.nanmax(n1) >= 0.9
    elif case == "stick":
        print(f"[observed] {task} stick: base speed along the surface after the last sub-step < {speed.max():.3f} m/s, median |f_t| / mu f_n {np.nanmedian(last):.3f}")
        assert (speed < 0.15).all() and np.nanmedian(last) < 0.5 and np.isfinite(last).sum() >= N
    elif case == "frictionless":
        cf = c["plane_trace"][1][2].astype(np.float64)
        assert (mu == 0).all() and np.abs(cf.reshape(N, -1, 3)[..., :2]).max() < 1e-3 * np.abs(cf).max()
    else:
        # first sub-step from the designed state with and without the exported self-collision forces: their difference is the self part
        outs = []
        for wc in (True, False):
            o = OracleSim(p, c["model"], robot, c["w"], threads=8)
            o.set_terrain(c["terr"].heightsamples, c["terr"].env_origins)
            H.load_state(o, c["ramp"], c["dof"], c["desc"]["friction"])
            o.physics_substep(c["tau"], wc)
            outs.append(o.buf["contact_forces"].astype(np.float64).reshape(N, -1, 3) @ c["R"])
        ground, self_part = outs[1], outs[0] - outs[1]
        crossed = np.arange(N) % 3 == 0
        assert crossed[N - 1]
        L, K = robot.chain_len, robot.num_limbs
        leaf = {k: sorted({int(pt.report_body) for pt, j in zip(robot.limb_points[k], robot.limb_point_joint[k]) if j == L - 1}) for k in range(K)}
        both = np.zeros(N, bool)
        # A1: 5e4 N/m contacts (ANYmal 1e6) and 60 g feet -- its self-collision forces are newtons, not hundreds of newtons
        f_self, f_ground = (50.0, 10.0) if task != "a1" else (0.5, 1.0)
        for k in range(K):
            s = np.linalg.norm(self_part[:, leaf[k]], axis=2).max(axis=1)
            gz = ground[:, leaf[k], 2].max(axis=1)
            both |= (s > f_self) & (gz > f_ground)
        print(f"[observed] {task} crossed: {int(both[crossed].sum())} of {int(crossed.sum())} crossed envs carry a self-collision force and a ground "
              f"force on one leaf body; largest self-collision force elsewhere {np.abs(self_part[~crossed]).max():.3g} N")
        assert both[N - 1] and both[crossed].sum() >= 5
        assert np.abs(self_part[~crossed]).max() == 0.0
