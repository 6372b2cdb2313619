"""Designed cases for the post stage of the predator-prey games (csrc/lg_game_post.h, csrc/lg_dec_game_post.h) and their float64 answers.
CPU only: NumPy, no torch, no library.  tests/test_game_edges.py runs the cases through the float32 twins, tests/test_gpu_game_edges.py through
the seven kernels; both assert the same things.

A *launch* is one call of a post kernel: the launch parameters it overrides (``capture_dist``, ``env_radius``, ``half_fov`` are parameters of
the launch, not of an env) and a *table* of independent envs.  Every env leaves the predator where it is written (zero predator velocity),
has no low-level reset and is far from the time limit unless the row is about those, and every row whose visibility is asserted is an env
that is not done (the observation of a done env is taken after the reset, from the Philox placement).

The float64 answers follow the reference's definitions, computed from the float32 inputs:

    captured      = norm(prey_xy - predator_xy) <  capture_dist                      (high_level_game.py:197-198)
    prey_out      = norm(prey_xy - origin_xy)   >  env_radius                        (:208), the predator alike (:209)
    visible       = |acos(dot(f, rel) / (|f| |rel|))| <= half_fov                    (:431-449)
    f             = quat_apply(normalize((0, 0, z, w)), (1, 0, 0)) = (1 - 2 z^2, 2 w z, 0), the norm clamped at 1e-9

The angle is taken as atan2(|f x rel|, f . rel) -- the same angle, and accurate near 0 and pi where acos is not; rel = 0 gives NaN, which
compares false: occluded.

Bands.  A row carries, per quantity, the distance from the threshold within which its decision is left open:
``band_dist`` in ulp of the threshold (0 on the rows whose float32 arithmetic is exact, ``B_DIST_ULP`` on the ladders) and ``band_angle``
as a multiple of ``angle_band()`` (0 on the exact rows, 1 elsewhere).

B_DIST_ULP = 4: the two squares and their sum contribute half an ulp each, which the root halves (3/4 ulp of the distance; the subtractions
are exact on the ladders, where one agent sits on the origin), and the device's root adds one ulp.  Under 2 ulp, doubled.
angle_band() = 8 * the worst |float32 twin angle - float64 angle| over the field-of-view ladders: it comes from the two references, never from
the device; the factor leaves room for the device's 2.5-ulp quotient, its two 1-ulp roots and an acosf that is not correctly rounded."""
import functools

import numpy as np

F = np.float32
D = np.float64
HALF_FOV, CAPTURE, PRED_Z, PREY_Z, PI32 = F(1.20428 / 2.0), F(0.5), F(0.3), F(0.35), F(np.pi)
RADIUS = F(3.0)
MAX_LEN = 1000
TERMINATION = -0.5
B_DIST_ULP = 4.0
ANGLE_FACTOR = 8.0
TRIPLES = ((3, 4, 5), (5, 12, 13), (8, 15, 17), (7, 24, 25), (20, 21, 29))
SCALES = (1.0 / 8, 1.0 / 16, 1.0 / 32)
FAR = 192.0          # 3 * 2^6: a position's ulp there (2^-16) is 256 times that of a 0.5 m threshold (2^-24)
YAWS = (0.0, 0.7, -2.3)
FOV_RUNGS, FOV_SPAN, LADDER_SIDE = 257, 1.25e-5, 64


# ----------------------------------------------------------------------------- tables
def table(n, seed):
    """``n`` envs with the defaults: prey at the origin looking along +x, predator 2 m ahead, seeded observation history."""
    rng = np.random.default_rng(seed)
    obs = rng.uniform(-5, 5, (n, 19)).astype(F)
    obs[:, 12:16] = rng.integers(0, 2, (n, 4))
    t = dict(prey=np.tile(np.array([0, 0, PREY_Z], F), (n, 1)), quat=np.tile(np.array([0, 0, 0, 1], F), (n, 1)), pred=np.tile(np.array([2, 0, PRED_Z], F), (n, 1)),
             origin=np.zeros((n, 3), F), ll_reset=np.zeros(n, bool), ll_time_out=np.zeros(n, bool), ep_len=np.full(n, 5, np.int64),
             ep_step=rng.integers(0, 50, n).astype(np.int64), obs=obs, band_dist=np.zeros(n), band_angle=np.ones(n), vis_known=np.ones(n, bool),
             ladder=np.full(n, -1, np.int64))
    return t


def concat(tables):
    return {k: np.concatenate([t[k] for t in tables], axis=0) for k in tables[0]}


def yaw_quat(t, yaw):
    t["quat"][:, 2], t["quat"][:, 3] = np.sin(np.asarray(yaw, D) / 2), np.cos(np.asarray(yaw, D) / 2)


def forward64(quat):
    """The reference's yaw-forward vector in float64 from the float32 quaternion -> (f [N,3], its yaw [N])."""
    z, w = quat[:, 2].astype(D), quat[:, 3].astype(D)
    n = np.maximum(np.hypot(z, w), 1e-9)
    z, w = z / n, w / n
    f = np.stack((1 - 2 * z * z, 2 * w * z, np.zeros_like(z)), axis=1)
    return f, np.arctan2(f[:, 1], f[:, 0])


def angle64(prey, quat, pred):
    f, _ = forward64(quat)
    rel = pred.astype(D) - prey.astype(D)
    dot, cross = (f * rel).sum(axis=1), np.linalg.norm(np.cross(f, rel), axis=1)
    return np.where((rel == 0).all(axis=1), np.nan, np.arctan2(cross, dot))


def game_state(t):
    """The table as the state dict of ``game_twin.post``."""
    n = t["prey"].shape[0]
    root = np.zeros((n, 13), F)
    root[:, :3], root[:, 3:7] = t["prey"], t["quat"]
    return dict(command=np.zeros((n, 6), F), root_states=root, env_origins=t["origin"].copy(), ll_rew=np.zeros(n, F), ll_reset=t["ll_reset"].copy(),
                predator_pos=t["pred"].copy(), obs=t["obs"].copy(), curr_episode_step=t["ep_step"].copy(), episode_length_buf=t["ep_len"].copy(),
                episode_sums=np.zeros((2, n), F))


def dec_state(t):
    """The table as the state dict of ``dec_game_twin.post``."""
    n = t["prey"].shape[0]
    s = game_state(t)
    del s["command"], s["obs"]
    s.update(command_pred=np.zeros((n, 2), F), dof_pos=np.zeros((n, 12), F), dof_vel=np.zeros((n, 12), F), obs_prey=t["obs"][:, :16].copy(),
             episode_sums=np.zeros((3, n), F), episode_means=np.zeros(3, F))
    return s


# ----------------------------------------------------------------------------- the groups
def _exact_offsets():
    """(dx, dy, hypotenuse) of every scaled triple in four placements; all dyadic."""
    out = []
    for a, b, c in TRIPLES:
        for s in SCALES:
            out += [(a * s, b * s, c * s), (b * s, a * s, c * s), (-a * s, b * s, c * s), (a * s, -b * s, c * s)]
    return np.array(out, D)


def hypotenuses():
    return sorted({c * s for _, _, c in TRIPLES for s in SCALES})


def exact_thresholds():
    """Every hypotenuse, and the float32 neighbour on either side of it."""
    out = []
    for h in hypotenuses():
        out += [F(h), np.nextafter(F(h), F(0)), np.nextafter(F(h), F(np.inf))]
    return out


def _exact_table(mode):
    """Every offset at origin 0 and at the far origin.  ``capture``: prey on the origin, predator offset.  ``radius``: half of the rows move the
    prey off the origin of its env and leave the predator on it, the other half the reverse."""
    off = _exact_offsets()
    rows = []
    for k, org in enumerate((0.0, FAR)):
        t = table(len(off), seed=10 + k)
        t["origin"][:, :2] = org
        t["prey"][:, :2] = org
        t["pred"][:, :2] = org
        move_prey = (np.arange(len(off)) % 2 == k) if mode == "radius" else np.zeros(len(off), bool)
        t["prey"][move_prey, :2] += off[move_prey, :2].astype(F)
        t["pred"][~move_prey, :2] += off[~move_prey, :2].astype(F)
        t["vis_known"][:] = False          # closer than 2 m: not a visibility row
        rows.append(t)
    return concat(rows)


def exact_launches():
    """One launch per threshold value: ``capture_dist`` (radius off) or ``env_radius`` (``capture_dist`` 0) is a hypotenuse or its neighbour."""
    out = []
    for T in exact_thresholds():
        out.append(dict(name=f"exact_capture_{float(T)!r}", family="both", over=dict(capture_dist=float(T), env_radius=-1.0), t=_exact_table("capture"), ladders=[], exact=True))
        out.append(dict(name=f"exact_radius_{float(T)!r}", family="game", over=dict(capture_dist=0.0, env_radius=float(T)), t=_exact_table("radius"), ladders=[], exact=True))
    return out


def _distance_ladder(lid, T, move, seed):
    """``move`` (prey or predator) at (ax, 0.3) from the origin, the other on it; ax one float per rung, LADDER_SIDE rungs on either side of
    the float64 crossing of the distance T."""
    y = F(0.3)
    ax0 = F(np.sqrt(D(T) ** 2 - D(y) ** 2))
    ax = [ax0]
    for _ in range(LADDER_SIDE):
        ax.append(np.nextafter(ax[-1], F(np.inf)))
    lo = [ax0]
    for _ in range(LADDER_SIDE):
        lo.append(np.nextafter(lo[-1], F(0)))
    ax = np.array(lo[:0:-1] + ax, F)
    t = table(len(ax), seed)
    other = "pred" if move == "prey" else "prey"
    t[move][:, 0], t[move][:, 1] = ax, y
    t[other][:, :2] = 0
    t["band_dist"][:], t["ladder"][:], t["vis_known"][:] = B_DIST_ULP, lid, False
    return t


def ladder_launches():
    cap = dict(name="ladder_capture", family="both", over=dict(capture_dist=float(CAPTURE), env_radius=-1.0), t=_distance_ladder(0, CAPTURE, "pred", 20),
               ladders=[dict(id=0, quantity="dist", threshold=float(CAPTURE), unit="ulp")])
    rad = dict(name="ladder_radius", family="game", over=dict(capture_dist=0.0, env_radius=float(RADIUS)),
               t=concat([_distance_ladder(1, RADIUS, "prey", 21), _distance_ladder(2, RADIUS, "pred", 22)]),
               ladders=[dict(id=1, quantity="prey_r", threshold=float(RADIUS), unit="ulp"), dict(id=2, quantity="pred_r", threshold=float(RADIUS), unit="ulp")])
    return [cap, rad]


def fov_launch():
    """Six ladders: three yaws, the crossing at +half_fov and at -half_fov.  Planar range 2 m, the task's heights; the bearing is spread evenly
    over +-FOV_SPAN around the float64 crossing, positions computed in float64 and rounded to float32."""
    R = 2.0
    rows, ladders = [], []
    for i, yaw in enumerate(YAWS):
        for j, side in enumerate((1.0, -1.0)):
            lid = 10 + 2 * i + j
            t = table(FOV_RUNGS, seed=30 + lid)
            yaw_quat(t, np.full(FOV_RUNGS, yaw))
            _, yaw_eff = forward64(t["quat"])
            rz = D(PRED_Z) - D(PREY_Z)
            beta0 = np.arccos(np.cos(D(HALF_FOV)) * np.sqrt(R * R + rz * rz) / R)
            beta = side * (beta0 + np.linspace(-FOV_SPAN, FOV_SPAN, FOV_RUNGS))
            t["pred"][:, 0], t["pred"][:, 1] = R * np.cos(yaw_eff + beta), R * np.sin(yaw_eff + beta)
            t["ladder"][:] = lid
            rows.append(t)
            ladders.append(dict(id=lid, quantity="angle", threshold=float(HALF_FOV), unit="rad"))
    return dict(name="fov_ladders", family="both", over=dict(capture_dist=float(CAPTURE), env_radius=-1.0, half_fov=float(HALF_FOV)), t=concat(rows), ladders=ladders)


def _ranges():
    return np.arange(32, 49) / 16.0          # 2 m .. 3 m in sixteenths: r and r * r are floats, the root of r * r is r


def _known_table():
    r = _ranges()
    n = len(r)
    ahead, behind = table(n, 40), table(n, 41)          # yaw 0, rz = 0: the acos argument is exactly +1 / -1
    for t, sgn in ((ahead, 1.0), (behind, -1.0)):
        t["prey"][:, 2] = PRED_Z
        t["pred"][:, 0] = sgn * r
        t["band_angle"][:] = 0
    tall = table(3 * n, 42)                                 # dead ahead with the task's height difference: atan(0.05 / r)
    yaw_quat(tall, np.repeat(YAWS, n))
    _, yaw_eff = forward64(tall["quat"])
    tall["pred"][:, 0], tall["pred"][:, 1] = np.tile(r, 3) * np.cos(yaw_eff), np.tile(r, 3) * np.sin(yaw_eff)
    side = table(4, 43)                                     # abeam on either side, and behind with the height difference
    side["pred"][:, :2] = [[0, 2], [0, -2], [-2, 0.25], [-2, -0.25]]
    return concat([ahead, behind, tall, side])


def known_launches():
    """The known angles under four fields of view: the task's, float32 pi, the float below it (acosf(-1) must be float32 pi) and 0."""
    out = []
    for name, hf in (("task", HALF_FOV), ("pi", PI32), ("below_pi", np.nextafter(PI32, F(0))), ("zero", F(0))):
        out.append(dict(name=f"known_{name}", family="both", over=dict(capture_dist=float(CAPTURE), env_radius=-1.0, half_fov=float(hf)), t=_known_table(), ladders=[]))
    return out


N_ARBITRARY = 1000


def degenerate_launch():
    """``capture_dist`` 0: nothing is captured.  Coincident prey and predator (0/0); rz = 0 with the predator exactly along the heading, at yaw 0
    over dyadic ranges (exact: visible) and at seeded arbitrary yaws (rounding decides between an argument of 1 and one past it: the truth
    "visible" is not demanded); a base quaternion with z = w = 0 (the clamp: forward is +x)."""
    same = table(3, 50)
    same["prey"][:, :2] = [[0, 0], [1.5, -2.25], [FAR, FAR]]
    same["pred"][:] = same["prey"]
    r = _ranges()
    along = table(len(r), 51)
    along["prey"][:, 2] = PRED_Z
    along["pred"][:, 0] = r
    along["band_angle"][:] = 0
    rng = np.random.default_rng(52)
    arb = table(N_ARBITRARY, 53)
    yaw_quat(arb, rng.uniform(-np.pi, np.pi, N_ARBITRARY))
    _, yaw_eff = forward64(arb["quat"])
    rr = rng.uniform(2.0, 6.0, N_ARBITRARY)
    arb["prey"][:, 2] = PRED_Z
    arb["pred"][:, 0], arb["pred"][:, 1] = rr * np.cos(yaw_eff), rr * np.sin(yaw_eff)
    arb["vis_known"][:] = False
    clamp = table(5, 54)
    clamp["quat"][:] = [[1, 0, 0, 0], [0.6, 0.8, 0, 0], [0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]]
    clamp["pred"][:, :2] = [[2, 0], [2, 0.5], [0, 2], [-2, 0], [2.5, 0]]
    return dict(name="degenerate", family="both", over=dict(capture_dist=0.0, env_radius=-1.0, half_fov=float(HALF_FOV)),
                t=concat([same, along, arb, clamp]), ladders=[], arbitrary=slice(3 + len(r), 3 + len(r) + N_ARBITRARY))


def dec_truth_launch():
    """capture x time limit x low-level reset x low-level time-out, five placements each.  ``scale_evasion_dt`` is 0 and the low-level reward
    0, so the prey's reward IS the termination term: exactly ``TERMINATION`` for a capture without time-out, exactly 0 otherwise."""
    combos = [(c, tl, lr, lt) for c in (0, 1) for tl in (0, 1) for lr in (0, 1) for lt in (0, 1)]
    place = [((0.0, 0.0), 0.0), ((FAR, FAR), 1.0), ((-40.0, 24.0), 2.5), ((3.0, -7.5), -0.7), ((FAR, -FAR), 3.0)]
    n = len(combos) * len(place)
    t = table(n, 60)
    for v, (org, ang) in enumerate(place):
        for k, (c, tl, lr, lt) in enumerate(combos):
            e = v * len(combos) + k
            d = 0.3 if c else 2.0
            t["origin"][e, :2] = org
            t["prey"][e, :2] = org
            t["pred"][e, :2] = (org[0] + d * np.cos(ang), org[1] + d * np.sin(ang))
            t["ep_len"][e] = MAX_LEN if tl else MAX_LEN - 1
            t["ll_reset"][e], t["ll_time_out"][e] = bool(lr), bool(lt)
    t["vis_known"][:] = False
    return dict(name="dec_truth", family="dec", over=dict(capture_dist=float(CAPTURE), half_fov=float(HALF_FOV), max_episode_length=MAX_LEN,
                                                          scale_termination_prey_dt=TERMINATION, scale_evasion_dt=0.0, only_positive_rewards_prey=1),
                t=t, ladders=[])


def outcome_truth_launch():
    """captured x prey out x predator out x low-level reset x low-level time-out for ``k_outcome_post``, three placements each, all well
    clear of the thresholds (capture 0.5 m, radius 3 m)."""
    geo = {(0, 0, 0): (1.0, -1.0), (0, 0, 1): (1.0, 1.3), (1, 0, 0): (3.5, 1.0), (1, 0, 1): (3.1, 2.8),          # (prey out, predator out, captured):
           (0, 1, 0): (1.0, 3.5), (0, 1, 1): (2.8, 3.1), (1, 1, 0): (3.5, -3.5), (1, 1, 1): (3.5, 3.8)}           # signed radii of prey and predator
    combos = [(g, lr, lt) for g in geo for lr in (0, 1) for lt in (0, 1)]
    place = [((0.0, 0.0), 0.0), ((FAR, FAR), 1.0), ((-40.0, 24.0), 2.5)]
    t = table(len(combos) * len(place), 61)
    for v, (org, ang) in enumerate(place):
        for k, (g, lr, lt) in enumerate(combos):
            e = v * len(combos) + k
            a, b = geo[g]
            t["origin"][e, :2] = org
            t["prey"][e, :2] = (org[0] + a * np.cos(ang), org[1] + a * np.sin(ang))
            t["pred"][e, :2] = (org[0] + b * np.cos(ang), org[1] + b * np.sin(ang))
            t["ll_reset"][e], t["ll_time_out"][e] = bool(lr), bool(lt)
    t["vis_known"][:] = False
    t["band_dist"][:] = B_DIST_ULP
    return dict(name="outcome_truth", family="game", over=dict(capture_dist=float(CAPTURE), env_radius=float(RADIUS), half_fov=float(HALF_FOV)), t=t, ladders=[])


@functools.lru_cache(maxsize=None)
def launches():
    """Every launch, by name."""
    out = exact_launches() + ladder_launches() + [fov_launch()] + known_launches() + [degenerate_launch(), dec_truth_launch(), outcome_truth_launch()]
    return {L["name"]: L for L in out}


def names(family):
    """The launches a kernel family (``game`` or ``dec``) runs."""
    return [k for k, L in launches().items() if L["family"] in ("both", family)]


# ----------------------------------------------------------------------------- float64 answers
@functools.lru_cache(maxsize=None)
def angle_band():
    """B_angle [rad]: ANGLE_FACTOR * the worst |float32 twin angle - float64 angle| over the field-of-view ladders."""
    from tests import game_twin as tw
    L = fov_launch()
    s = game_state(L["t"])
    _, _, angle, _, _ = tw.sense(tw.params(**L["over"]), s["predator_pos"], s["root_states"][:, :3], s["root_states"][:, 3:7], s["obs"][:, 9:12])
    return ANGLE_FACTOR * float(np.abs(np.abs(angle.astype(D)) - angle64(L["t"]["prey"], L["t"]["quat"], L["t"]["pred"])).max())


def truth(L, family):
    """The float64 answers of launch ``L`` for a kernel family: the quantities, the flags, and per flag the rows on which it is decided
    (further than the row's band from the threshold; a band of 0 decides every row)."""
    t, o = L["t"], L["over"]
    prey, pred, org = t["prey"].astype(D), t["pred"].astype(D), t["origin"].astype(D)
    cd, hf = D(F(o["capture_dist"])), D(F(o["half_fov"])) if "half_fov" in o else D(HALF_FOV)
    radius = D(F(o.get("env_radius", -1.0))) if family == "game" else -1.0
    a = dict(dist=np.hypot(*(prey[:, :2] - pred[:, :2]).T), prey_r=np.hypot(*(prey[:, :2] - org[:, :2]).T), pred_r=np.hypot(*(pred[:, :2] - org[:, :2]).T),
             angle=angle64(t["prey"], t["quat"], t["pred"]))
    n = len(a["dist"])

    def decided(q, T, band):
        return (band == 0) | (np.abs(q - T) > band)
    a["captured"], a["captured_decided"] = a["dist"] < cd, decided(a["dist"], cd, t["band_dist"] * np.spacing(F(cd)))
    if radius >= 0:
        band = t["band_dist"] * np.spacing(F(radius))
        a["prey_out"], a["prey_out_decided"] = a["prey_r"] > radius, decided(a["prey_r"], radius, band)
        a["pred_out"], a["pred_out_decided"] = a["pred_r"] > radius, decided(a["pred_r"], radius, band)
    else:
        a["prey_out"] = a["pred_out"] = np.zeros(n, bool)
        a["prey_out_decided"] = a["pred_out_decided"] = np.ones(n, bool)
    with np.errstate(invalid="ignore"):
        a["visible"] = np.abs(a["angle"]) <= hf          # NaN: False
        a["visible_decided"] = t["vis_known"] & (np.isnan(a["angle"]) | decided(a["angle"], hf, t["band_angle"] * (angle_band() if t["band_angle"].any() else 0.0)))
    a["time_out"] = (t["ep_len"] + 1 > int(o.get("max_episode_length", MAX_LEN))) if family == "dec" else np.zeros(n, bool)
    a["fell"], a["ll_timed_out"] = t["ll_reset"] & ~t["ll_time_out"], t["ll_reset"] & t["ll_time_out"]
    a["done"] = a["captured"] | a["prey_out"] | a["pred_out"] | a["time_out"] | t["ll_reset"]
    a["done_decided"] = a["captured_decided"] & a["prey_out_decided"] & a["pred_out_decided"]
    a["termination"] = np.where(a["captured"] & ~a["time_out"], F(o.get("scale_termination_prey_dt", 0.0)), F(0)).astype(F)
    steps = int((t["ep_step"][a["done"]] + 1).sum())
    if family == "game":          # lg_game_outcome: episodes, captured, prey_out, predator_out, fell, survived, steps
        a["counts"] = np.array([a["done"].sum(), a["captured"].sum(), a["prey_out"].sum(), a["pred_out"].sum(), a["fell"].sum(), a["ll_timed_out"].sum(), steps], np.int64)
    else:                         # lg_dec_game_outcome: episodes, captured, timed_out, fell, ll_timed_out, steps
        a["counts"] = np.array([a["done"].sum(), a["captured"].sum(), a["time_out"].sum(), a["fell"].sum(), a["ll_timed_out"].sum(), steps], np.int64)
    return a


# ----------------------------------------------------------------------------- the assertions, shared by the CPU and the device test
def check(L, family, out, info=None):
    """``out`` (a twin's or a kernel's result on launch ``L``) against the float64 answers -> dict of ladder id -> flip distance.

    - ``reset_buf`` equals the float64 decision on every row where that is decided; ``time_out_buf`` (dec) exactly.
    - On the rows that are decided to go on: the visibility flag equals the float64 decision where the angle is decided; the flag is 0 or 1, the
      observation finite, the history shifted; a visible row carries ``rel`` bit for bit, an occluded one repeats the previous newest sensed
      position; the other agent's observation is ``prey - predator``; predator and prey stay where they were written.
    - Every reward is finite; the prey's reward of the dec truth table is the termination term exactly.
    ``info``: the twin's info dict; with it the twin's own distance on the exact rows is held to the float64 one bit for bit."""
    t, a = L["t"], truth(L, family)
    obs_key = "obs" if family == "game" else "obs_prey"
    reset, obs = np.asarray(out["reset_buf"]).astype(bool), out[obs_key]
    dd = a["done_decided"]
    bad = np.nonzero(dd & (reset != a["done"]))[0]
    assert len(bad) == 0, (L["name"], "reset_buf", bad[:8].tolist(), a["dist"][bad[:8]].tolist(), a["prey_r"][bad[:8]].tolist(), a["pred_r"][bad[:8]].tolist())
    if family == "dec":
        np.testing.assert_array_equal(np.asarray(out["time_out_buf"]).astype(bool), a["time_out"], err_msg=L["name"])
        for k in ("rew_prey", "rew_pred"):
            assert np.isfinite(out[k]).all(), (L["name"], k)
        if L["name"] == "dec_truth":
            np.testing.assert_array_equal(out["rew_prey"].view(np.uint32), a["termination"].view(np.uint32), err_msg="termination term")
    else:
        assert np.isfinite(out["rew"]).all(), L["name"]
    on = dd & ~a["done"]
    assert not reset[on].any()
    flag = obs[on, 15]
    assert np.isin(flag, (0.0, 1.0)).all() and np.isfinite(obs[on]).all(), L["name"]
    vis = flag == 1
    vd = a["visible_decided"][on]
    bad = np.nonzero(vd & (vis != a["visible"][on]))[0]
    assert len(bad) == 0, (L["name"], "visible", np.nonzero(on)[0][bad[:8]].tolist(), a["angle"][on][bad[:8]].tolist())
    old = t["obs"][on]
    rel = (t["pred"][on] - t["prey"][on]).astype(F)
    np.testing.assert_array_equal(obs[on, 0:9].view(np.uint32), old[:, 3:12].view(np.uint32), err_msg=L["name"])
    np.testing.assert_array_equal(obs[on, 12:15].view(np.uint32), old[:, 13:16].view(np.uint32), err_msg=L["name"])
    np.testing.assert_array_equal(obs[on, 9:12].view(np.uint32), np.where(vis[:, None], rel, old[:, 9:12]).view(np.uint32), err_msg=L["name"])
    other = obs[on, 16:19] if family == "game" else out["obs_pred"][on]
    np.testing.assert_array_equal(other.view(np.uint32), (t["prey"][on] - t["pred"][on]).astype(F).view(np.uint32), err_msg=L["name"])
    np.testing.assert_array_equal(out["predator_pos"][on].view(np.uint32), t["pred"][on].view(np.uint32), err_msg=L["name"])
    np.testing.assert_array_equal(out["root_states"][on, :3].view(np.uint32), t["prey"][on].view(np.uint32), err_msg=L["name"])
    if info is not None and L.get("exact"):
        for k in ("dist_xy", "prey_r", "pred_r"):
            if k in info:
                q = a["dist" if k == "dist_xy" else k]
                assert (q.astype(F).astype(D) == q).all()
                np.testing.assert_array_equal(info[k].view(np.uint32), q.astype(F).view(np.uint32), err_msg=f"{L['name']}: {k}")
    flips = {}
    for lad in L["ladders"]:
        rows = np.nonzero(t["ladder"] == lad["id"])[0]
        q, T = a[lad["quantity"]][rows], lad["threshold"]
        if lad["quantity"] == "angle":
            got, want = np.zeros(len(rows), bool), a["visible"][rows]
            got[~reset[rows]] = obs[rows][~reset[rows], 15] == 1
            wrong = (got != want) & ~reset[rows]
        else:
            got = reset[rows]
            wrong = got != a["done"][rows]
        unit = float(np.spacing(F(T))) if lad["unit"] == "ulp" else 1.0
        flips[lad["id"]] = dict(quantity=lad["quantity"], unit=lad["unit"], distance=float(np.abs(q[wrong] - T).max() / unit) if wrong.any() else 0.0,
                                wrong=int(wrong.sum()), decisions=got)
    return flips


def ladder_conditions(L, family, flips):
    """What makes a ladder a test, asserted on the references alone: at most a quarter of the rungs inside the band, at least 16 decided
    rungs on either side, and the float32 twin's decisions flip exactly once along the ladder."""
    t, a, inside = L["t"], truth(L, family), {}
    for lad in L["ladders"]:
        rows = np.nonzero(t["ladder"] == lad["id"])[0]
        key = {"dist": "captured", "prey_r": "prey_out", "pred_r": "pred_out", "angle": "visible"}[lad["quantity"]]
        dec, ans = a[key + "_decided"][rows], a[key][rows]
        assert (~dec).sum() <= len(rows) // 4, (lad, int((~dec).sum()))
        assert (dec & ans).sum() >= 16 and (dec & ~ans).sum() >= 16, lad
        got = flips[lad["id"]]["decisions"]
        assert int((got[1:] != got[:-1]).sum()) == 1, (lad, np.nonzero(got[1:] != got[:-1])[0].tolist())
        inside[lad["id"]] = int((~dec).sum())
    return inside
