#!/usr/bin/env python3
"""Generate the game-layer fixtures under tests/golden/ (run in the build container only; needs the reference tree).

game_configs.json     -- ``class_to_dict`` of the reference's OWN ``HighLevelGameFlatCfg / HighLevelGameFlatCfgPPO``, obtained by executing
                         legged_gym/envs/a1_game/high_level_game_flat_config.py under the synthetic ``legged_gym`` package of tools/make_golden.py.
game_step.npz         -- inputs + outputs of the reference's OWN ``HighLevelGame.step`` (high_level_game.py:146-241) and everything it calls:
                         the clip block, ``step_predator_single_integrator``, ``_update_agent_states``, ``compute_reward`` + ``_reward_*``, the done
                         logic, ``reset_idx``, ``compute_observations``, ``sense_predator``, with ``_parse_cfg`` / ``_prepare_reward_function`` for
                         the scales.  The method bodies are extracted with ``ast`` at generation time (nothing is copied into this repo).  Only the
                         low-level env is a stand-in: its ``step`` installs the call's synthetic prey states / rewards / dones, its
                         ``_reset_root_states`` is the reference's ``LowLevelGame._reset_root_states`` (low_level_game.py:401-451), the gym
                         calls are no-ops, and every random draw is answered from the keyed Philox streams (``KeyedDraws``) under the purposes
                         GAME_ROOT = 16 / GAME_PREDATOR = 17.  Two sequences of consecutive calls on N = 512 envs: ``a`` (registered task,
                         env_radius None) and ``b`` (env_radius set).
                         One deliberate difference is built into the stand-in: ``ll_env.base_quat`` is served from
                         ``root_states`` at read time, i.e. AFTER the resets of the step, where the reference's low-level env would hand out the
                         quaternion it cached before them.
game_reset.npz        -- ``LowLevelGame._reset_root_states`` alone, with both ``custom_origins`` settings.
game_provenance.json  -- per fixture, the SHA-256 of every reference file executed (the format of provenance.json).

Env 0 is kept occluded and alive in every call.  The reference's ``sense_predator`` flattens a [n, 2] index table (:457), so row 0 always lands among its
"occluded" rows and env 0 repeats its previous sensed position whenever any env is occluded, whatever its own flag says; the build does not
reproduce that accident, and an occluded env 0 is the input on which both agree.

Inputs keep clear of the three thresholds (tests/game_twin.py: ``margins``): an env whose angle / capture distance / radius / |rel| is inside
the margin is redrawn before the reference runs."""
import ast
import json
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import make_golden as mg                                   # noqa: E402
from tests import game_twin as tw                          # noqa: E402
from tests import philox_np as ph                          # noqa: E402

HLG = "legged_gym/envs/a1_game/high_level_game.py"
LLG = "legged_gym/envs/a1_game/low_level_game.py"
CFG = "legged_gym/envs/a1_game/high_level_game_flat_config.py"
N = 512
F = np.float32


def record_provenance(*fixtures):
    path = os.path.join(mg.OUT, "game_provenance.json")
    table = json.load(open(path)) if os.path.isfile(path) else {}
    for f in fixtures:
        table[f] = dict(sorted(mg.EXECUTED.items()))
    with open(path, "w") as fh:
        json.dump(dict(sorted(table.items())), fh, indent=1)


def load_game_configs():
    """(HighLevelGameFlatCfg, HighLevelGameFlatCfgPPO, the locomotion config table) executed from the reference files."""
    base = mg.load_reference_configs()
    m = types.ModuleType("legged_gym.envs.a1_game.high_level_game_flat_config")
    path, text = mg.read_reference(CFG)
    m.__file__ = path
    m.__dict__["__builtins__"] = mg.SAFE_BUILTINS
    exec(compile(text, path, "exec"), m.__dict__)
    return m.HighLevelGameFlatCfg, m.HighLevelGameFlatCfgPPO, base


def configs():
    mg.EXECUTED.clear()
    E, T, _ = load_game_configs()
    out = {"high_level_game": {"env": mg.ref_class_to_dict(E()), "train": mg.ref_class_to_dict(T())}}
    with open(os.path.join(mg.OUT, "game_configs.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=False)
    record_provenance("game_configs.json")
    print("game_configs.json:", out["high_level_game"]["env"]["env"])


# ----------------------------------------------------------------------------- the reference's methods on stand-in objects
class _Draws:
    """Two keyed streams: torch_rand_float -> GAME_ROOT, Tensor.uniform_ / torch.rand -> GAME_PREDATOR."""

    def __init__(self):
        self.root = self.pred = None

    def begin(self, seed, step, env_ids, custom_origins):
        self.root, self.pred = mg.KeyedDraws(seed, step), mg.KeyedDraws(seed, step)
        self.root.enter(tw.GAME_ROOT, env_ids, 0 if custom_origins else 2)        # lanes 0-1 are the xy offset of custom origins
        self.pred.enter(tw.GAME_PREDATOR, env_ids, 0)


class _patched_torch:
    """``Tensor.uniform_`` and ``torch.rand`` answered from the keyed predator stream for the duration of a reference call."""

    def __init__(self, draws):
        self.draws = draws

    def __enter__(self):
        import torch
        d = self.draws
        self.saved = (torch.Tensor.uniform_, torch.rand)

        def uniform_(t, lo=0.0, hi=1.0):
            n, m = t.shape
            return t.copy_((hi - lo) * torch.from_numpy(d.pred.take(n, m)) + lo)

        def rand(n, **kw):
            return torch.from_numpy(d.pred.take(n, 1))[:, 0].clone()
        torch.Tensor.uniform_, torch.rand = uniform_, rand

    def __exit__(self, *exc):
        import torch
        torch.Tensor.uniform_, torch.rand = self.saved


def build_objects(radius, custom_origins, origins):
    """(high-level object with the reference's HighLevelGame methods, low-level stand-in with the reference's _reset_root_states, draws, namespace)."""
    import torch
    draws = _Draws()

    def torch_rand_float(lower, upper, shape, device):
        n, m = shape
        return (upper - lower) * torch.from_numpy(draws.root.take(n, m)) + lower

    ns = {"torch": torch, "np": np, "print": lambda *a, **k: None, "gymtorch": types.SimpleNamespace(unwrap_tensor=lambda t: t)}
    ns.update(mg._external_helpers())
    ns["torch_rand_float"] = torch_rand_float
    ns.update(mg._ref_functions("legged_gym/utils/math.py", None, ns, lambda k: k in ("quat_apply_yaw", "wrap_to_pi")))
    ns.update(mg._ref_functions("legged_gym/utils/helpers.py", None, ns, lambda k: k == "class_to_dict"))
    E, T, base = load_game_configs()
    a1_cfg = base["a1"][0]()

    ll_methods = mg._ref_functions(LLG, "LowLevelGame", ns, lambda k: k == "_reset_root_states")

    class LowLevelStandIn:
        _reset_root_states = ll_methods["_reset_root_states"]

        @property
        def base_quat(self):                    # the deliberate difference: the quaternion AFTER this step's resets
            return self.root_states[self.prey_indices, 3:7]

        def get_observations(self):
            return torch.zeros(self.num_envs, 1)

        def step(self, actions):
            k = self.call
            self.root_states[self.prey_indices] = self.feed["root_states"][k]
            return None, None, self.feed["ll_rew"][k].clone(), self.feed["ll_dones"][k].clone(), {}

    ll = LowLevelStandIn()
    ll.num_envs, ll.device = N, "cpu"
    ll.cfg, ll.dt = a1_cfg, a1_cfg.control.decimation * a1_cfg.sim.dt
    ll.root_states = torch.zeros(2 * N, 13)
    ll.prey_indices, ll.predator_indices = torch.arange(0, 2 * N, 2), torch.arange(1, 2 * N, 2)
    ll.custom_origins = bool(custom_origins)
    ll.env_origins = torch.from_numpy(origins).clone()
    i = a1_cfg.init_state
    ll.base_init_state = torch.tensor(list(i.pos) + list(i.rot) + list(i.lin_vel) + list(i.ang_vel), dtype=torch.float)
    ll.forward_vec = torch.tensor([1.0, 0.0, 0.0]).repeat(N, 1)
    ll.gym, ll.sim = types.SimpleNamespace(set_actor_root_state_tensor=lambda *a: None, set_actor_root_state_tensor_indexed=lambda *a: None), None

    keep = mg._ref_functions(HLG, "HighLevelGame", ns, lambda k: k.startswith("_reward_") or k in (
        "step", "step_predator_single_integrator", "reset_idx", "compute_reward", "compute_observations", "sense_predator", "_update_agent_states",
        "_prepare_reward_function", "_parse_cfg"))
    Ref = type("ReferenceHighLevelGameMethods", (), keep)
    env = Ref()
    env.cfg = E()
    env.cfg.env.env_radius = radius
    env.ll_env, env.ll_policy = ll, (lambda obs: obs)
    env.device, env.num_envs = "cpu", N
    env.capture_dist, env.MAX_REL_POS = env.cfg.env.capture_dist, 100.
    env._parse_cfg(env.cfg)
    env._prepare_reward_function()
    env.privileged_obs_buf, env.extras = None, {}
    return env, ll, draws, ns


def twin_params(env, ll, seed):
    return tw.params(num_envs=N, decimation=int(ll.cfg.control.decimation), heading_command=int(bool(env.cfg.commands.heading_command)),
                     only_positive_rewards=int(bool(env.cfg.rewards.only_positive_rewards)), custom_origins=int(ll.custom_origins), seed=int(seed),
                     cmd_lin_vel_x=tuple(env.command_ranges["lin_vel_x"]), cmd_lin_vel_y=tuple(env.command_ranges["lin_vel_y"]),
                     predator_lin_vel_x=tuple(env.command_ranges["predator_lin_vel_x"]), predator_lin_vel_y=tuple(env.command_ranges["predator_lin_vel_y"]),
                     capture_dist=float(env.capture_dist), env_radius=-1.0 if env.cfg.env.env_radius is None else float(env.cfg.env.env_radius),
                     half_fov=1.20428 / 2., max_rel_pos=float(env.MAX_REL_POS), ll_rew_weight=2.0,
                     scale_evasion_dt=float(env.reward_scales["evasion"]), scale_pursuit_dt=float(env.reward_scales["pursuit"]),
                     sim_dt=float(ll.cfg.sim.dt), predator_z=0.3, base_init_state=tuple(float(v) for v in ll.base_init_state))


def grid_origins(n, spacing=3.0):
    cols = int(np.floor(np.sqrt(n)))
    e = np.arange(n)
    return np.stack((spacing * (e // cols), spacing * (e % cols), np.zeros(n)), axis=1).astype(F)


def draw_inputs(rng, ids, pred_after, origins, radius):
    """Synthetic low-level outcome of one call for the envs ``ids``: prey root states placed relative to the (integrated) predator,
    most of them with the predator in front; ~12 % inside the capture distance; ~12 % reset by the low-level env."""
    n = len(ids)
    yaw = rng.uniform(-np.pi, np.pi, n)
    front = rng.random(n) < 0.6
    bearing = np.where(front, rng.uniform(-0.5, 0.5, n), rng.choice([-1.0, 1.0], n) * rng.uniform(0.75, np.pi, n))
    close = rng.random(n) < 0.12
    dist = np.where(close, rng.uniform(0.15, 0.45, n), rng.uniform(0.6, 5.0 if radius is not None else 8.0, n))
    root = np.zeros((n, 13), F)
    root[:, 0] = pred_after[ids, 0] - dist * np.cos(yaw + bearing)
    root[:, 1] = pred_after[ids, 1] - dist * np.sin(yaw + bearing)
    root[:, 2] = origins[ids, 2] + rng.uniform(0.25, 0.45, n)
    q = np.stack((rng.uniform(-0.08, 0.08, n), rng.uniform(-0.08, 0.08, n), np.sin(yaw / 2), np.cos(yaw / 2)), axis=1)
    root[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    root[:, 7:13] = rng.uniform(-1.0, 1.0, (n, 6))
    ll_rew = rng.uniform(-0.02, 0.05, n).astype(F)
    ll_dones = rng.random(n) < 0.12
    return root, ll_rew, ll_dones


def per_env_violations(p, info):
    bad = np.isnan(info["angle"]) | (np.abs(np.abs(info["angle"]) - F(p["half_fov"])) < 1.5e-3) | (np.abs(info["dist_xy"] - F(p["capture_dist"])) < 1.5e-4) \
        | (info["rel_norm"] < 1.5e-3)
    if p["env_radius"] >= 0:
        bad |= (np.abs(info["prey_r"] - F(p["env_radius"])) < 1.5e-4) | (np.abs(info["pred_r"] - F(p["env_radius"])) < 1.5e-4)
    return bad


def sequence(tag, radius, calls, seed, rng):
    import torch
    origins = grid_origins(N)
    env, ll, draws, ns = build_objects(radius, False, origins)
    p = tw.params(**twin_params(env, ll, seed))
    # initial state: predators a few metres from their origins, history at MAX_REL_POS as after construction (:121)
    pred0 = (origins + np.stack((rng.uniform(-2, 2, N), rng.uniform(-2, 2, N), np.full(N, 0.3)), axis=1)).astype(F)
    state = dict(predator_pos=pred0, obs=np.full((N, 19), 100.0, F), curr_episode_step=rng.integers(0, 50, N).astype(np.int64),
                 episode_length_buf=rng.integers(1, 50, N).astype(np.int64), episode_sums=np.zeros((2, N), F), env_origins=origins)
    ll.root_states[ll.predator_indices, :3] = torch.from_numpy(pred0)
    env.obs_buf = torch.from_numpy(state["obs"]).clone()
    env.rew_buf, env.reset_buf = torch.zeros(N), torch.ones(N, dtype=torch.long)
    env.curr_episode_step = torch.from_numpy(state["curr_episode_step"]).clone()
    env.episode_length_buf = torch.from_numpy(state["episode_length_buf"]).clone()
    env._update_agent_states()
    rec = {k: [] for k in ("in_command", "in_root_states", "in_ll_rew", "in_ll_dones", "step", "u_root", "u_pred", "command", "predator_integrated", "predator_pos",
                           "root_states", "obs", "rew", "reset_buf", "curr_episode_step", "episode_length_buf", "episode_sums", "sense_pos", "sense_flag")}
    ll.feed = {"root_states": [], "ll_rew": [], "ll_dones": []}
    inner_integrate, inner_sense = type(env).step_predator_single_integrator, type(env).sense_predator
    tap = {}

    def step_predator_single_integrator(self, command=None):
        inner_integrate(self, command=command)
        tap["predator_integrated"] = self.predator_pos.clone().numpy()

    def sense_predator(self):
        pos, flag = inner_sense(self)
        tap["sense_pos"], tap["sense_flag"] = pos.clone().numpy(), flag[:, 0].clone().numpy()
        return pos, flag
    type(env).step_predator_single_integrator, type(env).sense_predator = step_predator_single_integrator, sense_predator

    twin_state = dict(state)
    for k in range(calls):
        command = rng.uniform(-3.0, 3.0, (N, 6)).astype(F)
        command[:, 2] = rng.uniform(-9.0, 9.0, N)                           # beyond +-pi: the wrap of column 2
        clipped, _ = tw.pre(p, command)
        pred_after = tw.integrate_predator(p, twin_state["predator_pos"], clipped)
        root, ll_rew, ll_dones = draw_inputs(rng, np.arange(N), pred_after, origins, radius)
        for attempt in range(40):
            step_key = 1000 * (k + 1) + attempt
            for _ in range(30):
                s = dict(twin_state, command=clipped, root_states=root, ll_rew=ll_rew, ll_reset=ll_dones)
                out, info = tw.post(p, s, step=step_key)
                viol = per_env_violations(p, info)
                viol[0] |= bool(info["visible"][0]) or bool(out["reset_buf"][0])        # env 0 stays occluded and alive: see the module docstring
                bad = np.nonzero(viol)[0]
                if len(bad) == 0:
                    break
                command[bad] = rng.uniform(-3.0, 3.0, (len(bad), 6)).astype(F)             # (the predator's own position margin depends on its velocity)
                command[bad, 2] = rng.uniform(-9.0, 9.0, len(bad))
                clipped, _ = tw.pre(p, command)
                pred_after = tw.integrate_predator(p, twin_state["predator_pos"], clipped)
                r2, w2, d2 = draw_inputs(rng, bad, pred_after, origins, radius)
                root[bad], ll_rew[bad], ll_dones[bad] = r2, w2, d2
            if len(bad) == 0:
                break
        assert len(bad) == 0, "could not clear the threshold margins"
        tw.assert_margins(p, info)
        ll.call = k
        ll.feed["root_states"].append(torch.from_numpy(root).clone())
        ll.feed["ll_rew"].append(torch.from_numpy(ll_rew).clone())
        ll.feed["ll_dones"].append(torch.from_numpy(ll_dones).clone())
        done_ids = np.nonzero(out["reset_buf"])[0]
        draws.begin(seed, step_key, done_ids, False)
        cmd_t = torch.from_numpy(command).clone()
        with _patched_torch(draws):
            obs, _, rew, reset_buf, _ = env.step(cmd_t)                          # the reference's own step(), whole
        assert np.array_equal(np.nonzero(reset_buf.numpy())[0], done_ids), "twin and reference disagree on the done envs"
        u_root, u_pred = tw.draws(seed, N, step_key)
        rec["in_command"].append(command); rec["in_root_states"].append(root.copy()); rec["in_ll_rew"].append(ll_rew.copy()); rec["in_ll_dones"].append(ll_dones.copy())
        rec["step"].append(step_key); rec["u_root"].append(u_root); rec["u_pred"].append(u_pred)
        rec["command"].append(cmd_t.numpy().copy()); rec["predator_integrated"].append(tap["predator_integrated"])
        rec["predator_pos"].append(env.predator_pos.clone().numpy()); rec["root_states"].append(ll.root_states[ll.prey_indices].clone().numpy())
        rec["obs"].append(obs.clone().numpy()); rec["rew"].append(rew.clone().numpy()); rec["reset_buf"].append(reset_buf.clone().numpy())
        rec["curr_episode_step"].append(env.curr_episode_step.clone().numpy()); rec["episode_length_buf"].append(env.episode_length_buf.clone().numpy())
        rec["episode_sums"].append(np.stack([env.episode_sums[n_].clone().numpy() for n_ in ("evasion", "pursuit")]))
        rec["sense_pos"].append(tap["sense_pos"]); rec["sense_flag"].append(tap["sense_flag"])
        twin_state = {kk: out[kk] for kk in ("predator_pos", "obs", "curr_episode_step", "episode_length_buf", "episode_sums", "env_origins")}
        cap = info["capture"]
        print(f"  {tag} call {k}: step key {step_key}, visible {int(tap['sense_flag'].sum())}/{N}, captured {int(cap.sum())}, ll only {int((ll_dones & ~cap).sum())}, "
              f"both {int((ll_dones & cap).sum())}, radius {int(info['radius'].sum())}, neither {int((~out['reset_buf']).sum())}")
    res = {f"{tag}_{k}": np.stack(v) if k != "step" else np.array(v, np.int64) for k, v in rec.items()}
    res.update({f"{tag}_in0_{k}": state[k] for k in ("predator_pos", "obs", "curr_episode_step", "episode_length_buf", "episode_sums")})
    res[f"{tag}_env_origins"] = origins
    res[f"{tag}_params"] = np.array(json.dumps(p))
    return res


def step_fixture():
    mg.EXECUTED.clear()
    rng = np.random.default_rng(20)
    out = {}
    out.update(sequence("a", None, 4, seed=11, rng=rng))
    out.update(sequence("b", 6.0, 3, seed=12, rng=rng))
    out["base_quat_source"] = np.array("root_states at read time (after the step's resets)")
    out["env0"] = np.array("occluded and not done in every call")
    np.savez_compressed(os.path.join(mg.OUT, "game_step.npz"), **out)
    record_provenance("game_step.npz")
    print("game_step.npz written")


def reset_fixture():
    import torch
    mg.EXECUTED.clear()
    out = {}
    rng = np.random.default_rng(21)
    for custom in (0, 1):
        origins = grid_origins(N) if not custom else np.stack((rng.uniform(0, 80, N), rng.uniform(0, 160, N), rng.uniform(-0.5, 1.5, N)), axis=1).astype(F)
        env, ll, draws, ns = build_objects(None, custom, origins)
        seed, step = 31 + custom, 77 + 1000 * custom
        p = tw.params(**twin_params(env, ll, seed))
        ids = np.sort(rng.choice(N, N // 2, replace=False))
        before = rng.uniform(-5, 5, (2 * N, 13)).astype(F)
        ll.root_states[:] = torch.from_numpy(before)
        draws.begin(seed, step, ids, custom)
        with _patched_torch(draws):
            ll._reset_root_states(torch.from_numpy(ids))
        u_root, u_pred = tw.draws(seed, N, step)
        t = f"c{custom}"
        out.update({f"{t}_env_ids": ids, f"{t}_env_origins": origins, f"{t}_u_root": u_root, f"{t}_u_pred": u_pred, f"{t}_seed": np.int64(seed), f"{t}_step": np.int64(step),
                    f"{t}_in_root_states": before[0::2], f"{t}_in_predator_pos": before[1::2, :3],
                    f"{t}_root_states": ll.root_states[ll.prey_indices].clone().numpy(), f"{t}_predator_pos": ll.root_states[ll.predator_indices, :3].clone().numpy(),
                    f"{t}_params": np.array(json.dumps(p))})
        print(f"game_reset.npz: custom_origins={custom}: {len(ids)} of {N} envs reset")
    np.savez_compressed(os.path.join(mg.OUT, "game_reset.npz"), **out)
    record_provenance("game_reset.npz")


if __name__ == "__main__":
    which = sys.argv[1:] or ["configs", "step", "reset"]
    for w in which:
        {"configs": configs, "step": step_fixture, "reset": reset_fixture}[w]()
