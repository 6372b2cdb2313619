"""Cassie's natural fall as a test trajectory: set-ups, the action schedule, the CPU oracle's run and its event masks for the fall
tests (tests/test_cassie_fall.py on the CPU, tests/test_gpu_cassie_fall.py on the device).  Helpers only, no tests; NumPy and the
oracle only.

Cassie does not stand under zero actions.  Spawned 1 m up it falls for six policy steps, lands on its two-point toe capsules, stands
for a moment and topples until the pelvis meets the ground, which ends the episode (termination reward -200) and re-draws the env
inside the same step.  That one trajectory walks the step kernels k_step<CassieTraits, PD, plane | HF, NW> through everything the
quadruped tests do not reach: hard position limits on every joint, the speed limit, one and two toes down in the lanes of one
wave, the base contact point, the in-step reset and, on the height field, the terrain-curriculum level change.

N = 40 envs: CassieTraits has K = 2 limbs, so a workgroup holds 32 envs -- one full workgroup and a partial one with 8 live envs
(32..39) whose dead lanes replicate env 39.

Two set-ups ("plane" and "heightfield"), T = 48 policy steps each, the step counter equal to the step index:
- plane: tests/test_gpu_parity.init_both -- grid origins, randomize_env_params(N, 3), reset of every env at counter 0;
- heightfield: the 4 x 5 curriculum field of tests/test_gpu_parity._rough_terrain(N) (restated here: that module needs torch),
  spawned as tests/test_gpu_full_size._spawn with default_rng(0), friction (0.5, 1.25), mass (-1, 1), max_init_terrain_level 3.
Actions: zero for steps 1 to 16, then 0.3 * N(0, 1) drawn from default_rng([ACTION_SEED, step]).

[observed] with these seeds (SIM_SEED 6, ACTION_SEED 1), from the oracle alone; tests/test_cassie_fall.py asserts the conditions the
device test relies on.  (SIM_SEED: with seed 1 env 39 never resets within 48 steps, whatever the action seed; of the seeds up to 24 in
which it does, 6 has the widest margins under one ulp of input noise -- with 18 a toe of the height-field run sits on the 1 N contact
threshold at step 21.)
  plane        9 envs start step 1 beyond a hard limit (10 start step 2 so); airborne for steps 1 - 6, first toe contact at step 7; one-toe
               and two-toe envs in the same step in 34 steps (steps 7 - 12: 3 to 7 envs on one toe, 2 to 36 on two); all 40 envs on both
               toes in steps 16 and 17; first pelvis contact at step 21; 30 resets by step 48, all by base contact and every base contact
               a reset, rew_buf -4.07 .. -3.98; 7 of them in envs 32..39, env 39 at step 32; 309 one-toe env-steps; 6 env-steps end with a
               joint at its speed limit (one in step 1); no time-outs.
  heightfield  9 envs start step 1 beyond a hard limit; first toe contact at step 7; one-toe and two-toe envs in the same step in 35 steps;
               all 40 on both toes in step 17; 30 resets (first at step 21, rew_buf -4.14 .. -3.98), 7 in envs 32..39, env 39 at step 32;
               27 terrain-level changes, 7 in envs 32..39; 307 one-toe env-steps; 3 env-steps with a joint at its speed limit; no time-outs.
"""
import functools

import numpy as np

from tests.common import TASK_CFG, grid_origins, make_setup, randomize_env_params

N = 40
T = 48
ZERO_STEPS = 16                                  # steps 1 .. ZERO_STEPS take zero actions
ACTION_SEED = 1
SIM_SEED = 6                                     # lg_params.seed: the Philox key of every reset draw
WORKGROUP_ENVS = 32                              # CassieTraits: 64 lanes / K = 2
KINDS = ("plane", "heightfield")
FLAGS = ("reset_buf", "time_out_buf", "episode_length_buf", "terrain_levels", "last_contacts")


def rough_terrain(N_envs):
    """The curriculum field of tests/test_gpu_parity._rough_terrain (4 x 5 tiles of the anymal_c_rough terrain, seed 7)."""
    from legged_games_gym_amd.utils.terrain import Terrain
    tc = TASK_CFG["anymal_c_rough"]().terrain
    tc.mesh_type, tc.num_rows, tc.num_cols, tc.border_size = "heightfield", 4, 5, 5
    np.random.seed(7)
    return Terrain(tc, N_envs)


def fall_setup(kind, N_envs=N):
    """dict(kind, N, cfg, robot, p, model, w, terr) of Cassie on the plane or on the curriculum height field."""
    if kind == "plane":
        terr = None
        cfg, robot, p, names, model, w = make_setup("cassie", N_envs, seed=SIM_SEED)
    else:
        terr = rough_terrain(N_envs)

        def tweak(cfg):
            cfg.terrain.mesh_type, cfg.terrain.num_rows, cfg.terrain.num_cols, cfg.terrain.border_size = "heightfield", 4, 5, 5
            cfg.terrain.max_init_terrain_level = 3
        cfg, robot, p, names, model, w = make_setup("cassie", N_envs, seed=SIM_SEED, tweak=tweak, terrain=terr, plane=False)
        assert p.terrain_curriculum == 1 and p.hf_step_threshold == 0
    assert robot.num_limbs == 2 and robot.chain_len == 6 and robot.dof_has_limits.all() and p.push_interval > T
    return dict(kind=kind, N=N_envs, cfg=cfg, robot=robot, p=p, model=model, w=w, terr=terr)


def new_oracle(s, threads=8):
    from oracle.oracle import OracleSim
    o = OracleSim(s["p"], s["model"], s["robot"], s["w"], threads=threads)
    if s["terr"] is not None:
        o.set_terrain(s["terr"].heightsamples, s["terr"].env_origins)
    o.buf["cmd_range"][:] = list(s["p"].cmd_lin_vel_x)
    return o


def spawn_params(s):
    """The creation-time buffers of a set-up: {name: array} (env origins, friction, base mass and, on the field, levels / types)."""
    Nn, cfg, terr = s["N"], s["cfg"], s["terr"]
    if terr is None:
        fr, dm = randomize_env_params(Nn, 3)
        return dict(env_origins=grid_origins(Nn), friction_coeffs=fr, base_mass_delta=dm)
    rng = np.random.default_rng(0)                # the draws of tests/test_gpu_full_size._spawn, in its order
    buckets = rng.uniform(0.5, 1.25, 64).astype(np.float32)
    fr = buckets[rng.integers(0, 64, Nn)]
    dm = rng.uniform(-1.0, 1.0, Nn).astype(np.float32)
    lv = rng.integers(0, cfg.terrain.max_init_terrain_level + 1, Nn).astype(np.int32)
    ty = np.floor(np.arange(Nn) / (Nn / cfg.terrain.num_cols)).astype(np.int32)
    return dict(env_origins=terr.env_origins[lv, ty].astype(np.float32), friction_coeffs=fr, base_mass_delta=dm, terrain_levels=lv, terrain_types=ty)


def spawn(o, s):
    for k, v in spawn_params(s).items():
        o.buf[k][...] = v.reshape(o.buf[k].shape)
    o.reset_idx(np.arange(s["N"], dtype=np.int32), 0)


def actions_for(step, N_envs):
    if step <= ZERO_STEPS:
        return np.zeros((N_envs, 12), np.float32)
    return (0.3 * np.random.default_rng([ACTION_SEED, step]).standard_normal((N_envs, 12))).astype(np.float32)


def snapshot(o):
    return {k: v.copy() for k, v in o.buf.items()}


def load_state(o, state):
    """Every buffer of the oracle from a snapshot."""
    for k, v in state.items():
        o.buf[k][...] = v


def events(s, before, after):
    """Event masks of one policy step, [N] each: beyond_limit (a joint outside its hard limits BEFORE the step), at_vel_limit (a joint at
    dof_vel_limit after it), toes (0 / 1 / 2 toes with F_z > 1 N, the last_contacts rule), base (pelvis force > 1 N), reset, time_out,
    level (terrain level changed).  The forces of an env that reset are those that ended its episode."""
    robot, Nn = s["robot"], s["N"]
    q0 = before["dof_state"].reshape(Nn, 12, 2)[..., 0]
    qd1 = after["dof_state"].reshape(Nn, 12, 2)[..., 1]
    cf = after["contact_forces"].reshape(Nn, -1, 3)
    toes, pelvis = robot.bodies_matching("toe"), robot.bodies_matching("pelvis")
    assert len(toes) == 2 and pelvis[0] == 0       # 'pelvis' also names the two pelvis_rotation links, as in the termination mask
    ev = dict(beyond_limit=((q0 < robot.dof_lower.astype(np.float32)) | (q0 > robot.dof_upper.astype(np.float32))).any(axis=1),
              at_vel_limit=(np.abs(qd1) >= robot.dof_velocity.astype(np.float32)).any(axis=1),
              toes=(cf[:, toes, 2] > 1.0).sum(axis=1), base=(np.linalg.norm(cf[:, pelvis], axis=2) > 1.0).any(axis=1),
              reset=after["reset_buf"].astype(bool), time_out=after["time_out_buf"].astype(bool))
    ev["level"] = (after["terrain_levels"] != before["terrain_levels"]) if "terrain_levels" in after else np.zeros(Nn, bool)
    return ev


@functools.lru_cache(maxsize=None)
def trajectory(kind):
    """The oracle's run at N = 40: dict(setup, states [T + 1] (states[t - 1] is the complete o.buf before step t, states[t] after it),
    actions [T], events [T])."""
    s = fall_setup(kind)
    o = new_oracle(s)
    spawn(o, s)
    states, acts, evs = [snapshot(o)], [], []
    for t in range(1, T + 1):
        a = actions_for(t, N)
        o.step(a, t)
        states.append(snapshot(o))
        acts.append(a)
        evs.append(events(s, states[-2], states[-1]))
    return dict(setup=s, states=states, actions=acts, events=evs)


def stacked(tr, name):
    """[T, N] array of one event mask."""
    return np.stack([e[name] for e in tr["events"]])


def chosen_steps(N_envs, threads=16):
    """The plane run at N_envs envs, from the oracle alone, up to the last of three chosen steps: the first with at least 30 % of the
    envs on a toe ('landing'), step 16 ('stance') and the first from 20 on in which at least 0.5 % of the envs reset ('fall').
    Returns (setup, {name: dict(step, before, after, actions, contact_share)}), contact_share being the share of envs whose contact
    forces carry more than 50 N of F_z after the step (the rule of tests/test_gpu_full_size._compare_every_env)."""
    s = fall_setup("plane", N_envs)
    o = new_oracle(s, threads)
    spawn(o, s)
    out = {}
    for t in range(1, T + 1):
        a = actions_for(t, N_envs)
        before = snapshot(o)
        o.step(a, t)
        cf = o.buf["contact_forces"].reshape(N_envs, -1, 3)
        toes = (cf[:, s["robot"].bodies_matching("toe"), 2] > 1.0).any(axis=1).mean()
        name = None
        if "landing" not in out and toes >= 0.3:
            name = "landing"
        elif t == 16:
            name = "stance"
        elif t >= 20 and "fall" not in out and o.buf["reset_buf"].mean() >= 0.005:
            name = "fall"
        if name is not None:
            out[name] = dict(step=t, before=before, after=snapshot(o), actions=a, contact_share=float((np.abs(cf[..., 2]).sum(axis=1) > 50.0).mean()))
        if len(out) == 3:
            break
    assert set(out) == {"landing", "stance", "fall"} and out["landing"]["step"] < 16 < out["fall"]["step"], {k: v["step"] for k, v in out.items()}
    return s, out
