"""Shared helpers of the scripted-pursuer tests (CPU and device): the calls of tests/golden/pursuer_step.npz through the twin, and a seeded
synthetic state that keeps the threshold margins of tests/game_twin.py under the pursuer's own move."""
import json

import numpy as np

from tests import game_twin as tw
from tests import pursuer_twin as pt

F = np.float32
WANT = ("command", "predator_command", "ep", "predator_integrated", "predator_pos", "root_states", "obs", "rew", "reset_buf", "curr_episode_step",
        "episode_length_buf", "episode_sums", "sense_pos", "sense_flag")


def initial_state(g, tag):
    state = {k: g[f"{tag}_in0_{k}"] for k in ("predator_pos", "obs", "curr_episode_step", "episode_length_buf", "episode_sums")}
    state["env_origins"] = g[f"{tag}_env_origins"]
    return state


def call_inputs(g, tag, k, p, state):
    command, _ = tw.pre(p, g[f"{tag}_in_command"][k])
    return dict(state, command=command, root_states=g[f"{tag}_in_root_states"][k], ll_rew=g[f"{tag}_in_ll_rew"][k], ll_reset=g[f"{tag}_in_ll_dones"][k])


def pursuer_calls(g, tag):
    """Yield (k, params, pursuer params, twin input state, twin outputs, twin info, fixture outputs of call k).  The state is carried by the
    TWIN, with one exception: the episode sums enter call k + 1 as the fixture recorded them after call k.  The reference never zeroes them, so
    a surviving env adds one reward term per call, each behind a norm that torch and NumPy may round differently; carried by the twin, that
    difference grows with the number of calls (2 ulp of the sum after three calls here), while ``check_call``'s bound is that of ONE call."""
    p, q = json.loads(str(g[f"{tag}_params"])), json.loads(str(g[f"{tag}_pursuer_params"]))
    state = initial_state(g, tag)
    for k in range(g[f"{tag}_step"].shape[0]):
        s = call_inputs(g, tag, k, p, state)
        out, info = pt.post(p, q, s, u_root=g[f"{tag}_u_root"][k], u_pred=g[f"{tag}_u_pred"][k])
        yield k, p, q, s, out, info, {n: g[f"{tag}_{n}"][k] for n in WANT}
        state = {n: out[n] for n in ("predator_pos", "obs", "curr_episode_step", "episode_length_buf", "env_origins")}
        state["episode_sums"] = g[f"{tag}_episode_sums"][k]


def synthetic_state(p, q, n, seed, step):
    """Seeded state for ``lg_pursuer_post`` on ``n`` envs, redrawn until every env keeps the margins on the twin: the prey placed around the
    predator (some inside the capture distance, most with the predator in front), episode steps from [0, 1.3 L), some envs reset by the
    low-level env, some outside the radius when one is set.  Columns 4:6 of the command are random: the kernel must ignore them."""
    rng = np.random.default_rng(seed)
    cols = max(1, int(np.floor(np.sqrt(n))))
    e = np.arange(n)
    origins = np.stack((3.0 * (e // cols), 3.0 * (e % cols), np.zeros(n)), axis=1).astype(F)
    pred = (origins + np.stack((rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), np.full(n, 0.3)), axis=1)).astype(F)
    obs = rng.uniform(-5, 5, (n, 19)).astype(F)
    obs[:, 12:16] = rng.integers(0, 2, (n, 4))
    cmd = rng.uniform(-3.0, 3.0, (n, 6)).astype(F)
    cmd[:, 2] = rng.uniform(-9.0, 9.0, n)
    s = dict(predator_pos=pred, obs=obs, curr_episode_step=rng.integers(0, int(1.3 * q["max_episode_length"]), n).astype(np.int64),
             episode_length_buf=rng.integers(1, 50, n).astype(np.int64), episode_sums=rng.uniform(-1, 1, (2, n)).astype(F), env_origins=origins,
             command=tw.pre(p, cmd)[0], root_states=np.zeros((n, 13), F), ll_rew=np.zeros(n, F), ll_reset=np.zeros(n, bool))

    def draw(ids):
        m = len(ids)
        yaw = rng.uniform(-np.pi, np.pi, m)
        bearing = np.where(rng.random(m) < 0.6, rng.uniform(-0.5, 0.5, m), rng.choice([-1.0, 1.0], m) * rng.uniform(0.75, np.pi, m))
        dist = np.where(rng.random(m) < 0.12, rng.uniform(0.15, 0.45, m), rng.uniform(0.6, 6.0, m))
        root = np.zeros((m, 13), F)
        root[:, 0] = pred[ids, 0] - dist * np.cos(yaw + bearing)
        root[:, 1] = pred[ids, 1] - dist * np.sin(yaw + bearing)
        root[:, 2] = rng.uniform(0.25, 0.45, m)
        quat = np.stack((rng.uniform(-0.08, 0.08, m), rng.uniform(-0.08, 0.08, m), np.sin(yaw / 2), np.cos(yaw / 2)), axis=1)
        root[:, 3:7] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
        root[:, 7:13] = rng.uniform(-1.0, 1.0, (m, 6))
        s["root_states"][ids], s["ll_rew"][ids], s["ll_reset"][ids] = root, rng.uniform(-0.02, 0.05, m).astype(F), rng.random(m) < 0.12
    ids = e
    for attempt in range(200):
        draw(ids)
        if attempt:
            s["ll_reset"][ids] = False      # an env whose margin fails AFTER its reset cannot be fixed by new inputs alone: keep it alive
        out, info = pt.post(p, q, s, step=step)
        bad = np.isnan(info["angle"]) | (np.abs(np.abs(info["angle"]) - F(p["half_fov"])) < 2e-3) | (np.abs(info["dist_xy"] - F(p["capture_dist"])) < 2e-4) | (info["rel_norm"] < 2e-3)
        if p["env_radius"] >= 0:
            bad |= (np.abs(info["prey_r"] - F(p["env_radius"])) < 2e-4) | (np.abs(info["pred_r"] - F(p["env_radius"])) < 2e-4)
        ids = np.nonzero(bad)[0]
        if len(ids) == 0:
            return s
    raise AssertionError("could not draw a state that keeps the margins")
