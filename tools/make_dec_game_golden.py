#!/usr/bin/env python3
"""Generate the fixtures of the decentralised game under tests/golden/ (run in the build container only; needs the reference tree).

dec_game_configs.json     -- ``class_to_dict`` of the reference's OWN ``DecHighLevelGameCfg / DecHighLevelGameCfgPPO``, obtained by executing
                             legged_gym/envs/a1_game/dec_high_level_game_config.py under the synthetic ``legged_gym`` package of tools/make_golden.py.
dec_game_step.npz         -- inputs + outputs of the reference's OWN ``DecHighLevelGame.step`` (dec_high_level_game.py:169-210) and everything it
                             calls: the clip block, ``step_predator_single_integrator``, ``post_physics_step``, ``check_termination``, ``reset_idx``,
                             both ``compute_reward_*`` + the ``_reward_*`` functions, both ``compute_observations_*``, ``prey_sense_predator``,
                             ``_update_agent_states``, with ``_parse_cfg`` / both ``_prepare_reward_function_*`` for the scales.  The method bodies
                             are extracted with ``ast`` at generation time (nothing is copied into this repo) and their ``print`` calls are
                             silenced.  Only the low-level env is a stand-in, the one of tools/make_game_golden.py plus the joints: its ``step``
                             installs the call's synthetic prey states / rewards / dones, its ``_reset_dofs`` / ``_reset_root_states`` are the
                             reference's ``LowLevelGame`` methods (low_level_game.py:383-451), the gym calls are no-ops, and every random draw is
                             answered from the keyed Philox streams under the purposes GAME_ROOT = 16 / GAME_PREDATOR = 17 / GAME_DOF = 18.
                             Two sequences of consecutive calls on N = 512 envs: ``a`` (the registered task) and ``t`` (a prey ``termination``
                             scale set, so that :338-341 run).  Some envs start at ``max_episode_length - 1 .. + 1`` so that time-outs occur.
                             ``ll_env.base_quat`` is served from ``root_states`` at read time, as in tools/make_game_golden.py.
dec_game_provenance.json  -- per fixture, the SHA-256 of every reference file executed (the format of game_provenance.json).

Env 0 is kept occluded and alive in every call: ``prey_sense_predator`` flattens a [n, 2] index table (:447), so row 0 always lands among its
"occluded" rows; the build does not reproduce that accident, and an occluded env 0 is the input on which both agree.
Inputs keep clear of the thresholds (tests/game_twin.py: ``margins``): an env inside a margin is redrawn before the reference runs."""
import json
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import make_golden as mg                                   # noqa: E402
import make_game_golden as mgg                             # noqa: E402
from tests import dec_game_twin as dt                      # noqa: E402

DEC = "legged_gym/envs/a1_game/dec_high_level_game.py"
LLG = mgg.LLG
CFG = "legged_gym/envs/a1_game/dec_high_level_game_config.py"
N = mgg.N
F = np.float32
METHODS = ("step", "step_predator_single_integrator", "post_physics_step", "check_termination", "reset_idx", "compute_reward_prey", "compute_reward_pred",
           "compute_observations_pred", "compute_observations_prey", "prey_sense_predator", "_update_agent_states", "_parse_cfg",
           "_prepare_reward_function_pred", "_prepare_reward_function_prey")


def record_provenance(*fixtures):
    path = os.path.join(mg.OUT, "dec_game_provenance.json")
    table = json.load(open(path)) if os.path.isfile(path) else {}
    for f in fixtures:
        table[f] = dict(sorted(mg.EXECUTED.items()))
    with open(path, "w") as fh:
        json.dump(dict(sorted(table.items())), fh, indent=1)


def load_dec_configs():
    """(DecHighLevelGameCfg, DecHighLevelGameCfgPPO, the locomotion config table) executed from the reference files."""
    base = mg.load_reference_configs()
    m = types.ModuleType("legged_gym.envs.a1_game.dec_high_level_game_config")
    path, text = mg.read_reference(CFG)
    m.__file__ = path
    m.__dict__["__builtins__"] = mg.SAFE_BUILTINS
    exec(compile(text, path, "exec"), m.__dict__)
    return m.DecHighLevelGameCfg, m.DecHighLevelGameCfgPPO, base


def configs():
    mg.EXECUTED.clear()
    E, T, _ = load_dec_configs()
    out = {"dec_high_level_game": {"env": mg.ref_class_to_dict(E()), "train": mg.ref_class_to_dict(T())}}
    with open(os.path.join(mg.OUT, "dec_game_configs.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=False)
    record_provenance("dec_game_configs.json")
    print("dec_game_configs.json:", out["dec_high_level_game"]["env"]["env"])


class _Draws(mgg._Draws):
    """The two streams of tools/make_game_golden.py plus the joints: torch_rand_float of 12 columns -> GAME_DOF."""

    def begin(self, seed, step, env_ids, custom_origins):
        super().begin(seed, step, env_ids, custom_origins)
        self.dof = mg.KeyedDraws(seed, step)
        self.dof.enter(dt.GAME_DOF, env_ids, 0)


def build_objects(tweak=None):
    """(object with the reference's DecHighLevelGame methods, low-level stand-in with the reference's reset methods, draws)."""
    import torch
    draws = _Draws()

    def torch_rand_float(lower, upper, shape, device):
        n, m = shape
        stream = draws.dof if m == dt.NUM_DOF else draws.root
        return (upper - lower) * torch.from_numpy(stream.take(n, m)) + lower

    ns = {"torch": torch, "np": np, "print": lambda *a, **k: None, "gymtorch": types.SimpleNamespace(unwrap_tensor=lambda t: t)}
    ns.update(mg._external_helpers())
    ns["torch_rand_float"] = torch_rand_float
    ns.update(mg._ref_functions("legged_gym/utils/math.py", None, ns, lambda k: k in ("quat_apply_yaw", "wrap_to_pi")))
    ns.update(mg._ref_functions("legged_gym/utils/helpers.py", None, ns, lambda k: k == "class_to_dict"))
    E, T, base = load_dec_configs()
    a1_cfg = base["a1"][0]()
    ll_methods = mg._ref_functions(LLG, "LowLevelGame", ns, lambda k: k in ("_reset_dofs", "_reset_root_states"))

    class LowLevelStandIn:
        _reset_dofs = ll_methods["_reset_dofs"]
        _reset_root_states = ll_methods["_reset_root_states"]

        @property
        def base_quat(self):                    # the deliberate difference: the quaternion AFTER this step's resets
            return self.root_states[self.prey_indices, 3:7]

        def get_observations(self):
            return torch.zeros(self.num_envs, 1)

        def step(self, actions):
            k = self.call
            self.root_states[self.prey_indices] = self.feed["root_states"][k]
            self.reset_buf = self.feed["ll_dones"][k].clone()
            return None, None, self.feed["ll_rew"][k].clone(), self.feed["ll_dones"][k].clone(), {}

    ll = LowLevelStandIn()
    ll.num_envs, ll.device = N, "cpu"
    ll.cfg, ll.dt = a1_cfg, a1_cfg.control.decimation * a1_cfg.sim.dt
    ll.root_states = torch.zeros(2 * N, 13)
    ll.prey_indices, ll.predator_indices = torch.arange(0, 2 * N, 2), torch.arange(1, 2 * N, 2)
    ll.custom_origins = False
    i = a1_cfg.init_state
    ll.base_init_state = torch.tensor(list(i.pos) + list(i.rot) + list(i.lin_vel) + list(i.ang_vel), dtype=torch.float)
    ll.forward_vec = torch.tensor([1.0, 0.0, 0.0]).repeat(N, 1)
    ll.num_dof = dt.NUM_DOF
    ll.default_dof_pos = torch.tensor([float(v) for v in i.default_joint_angles.values()], dtype=torch.float).unsqueeze(0)
    assert ll.default_dof_pos.shape == (1, dt.NUM_DOF)
    ll.dof_state = torch.zeros(N, dt.NUM_DOF, 2)
    ll.dof_pos, ll.dof_vel = ll.dof_state[..., 0], ll.dof_state[..., 1]
    noop = lambda *a: None
    ll.gym, ll.sim = types.SimpleNamespace(set_actor_root_state_tensor=noop, set_actor_root_state_tensor_indexed=noop, set_dof_state_tensor_indexed=noop), None
    ll.reset_buf = torch.zeros(N, dtype=torch.bool)

    keep = mg._ref_functions(DEC, "DecHighLevelGame", ns, lambda k: k.startswith("_reward_") or k in METHODS)
    assert set(METHODS) <= set(keep)
    Ref = type("ReferenceDecHighLevelGameMethods", (), keep)
    env = Ref()
    env.cfg = E()
    if tweak:
        tweak(env.cfg)
    env.ll_env, env.ll_policy = ll, (lambda obs: obs)
    env.device, env.num_envs = "cpu", N
    env.capture_dist, env.MAX_REL_POS = env.cfg.env.capture_dist, 100.
    env._parse_cfg(env.cfg)
    env._prepare_reward_function_pred()
    env._prepare_reward_function_prey()
    env.privileged_obs_buf_pred = env.privileged_obs_buf_prey = None
    env.extras = {}
    return env, ll, draws


def twin_params(env, ll, seed):
    return dt.params(num_envs=N, decimation=int(ll.cfg.control.decimation), heading_command=int(bool(env.cfg.commands.heading_command)),
                     custom_origins=int(ll.custom_origins), only_positive_rewards_prey=int(bool(env.cfg.rewards_prey.only_positive_rewards)),
                     only_positive_rewards_pred=int(bool(env.cfg.rewards_predator.only_positive_rewards)), max_episode_length=int(env.max_episode_length),
                     seed=int(seed), cmd_lin_vel_x=tuple(env.command_ranges["lin_vel_x"]), cmd_lin_vel_y=tuple(env.command_ranges["lin_vel_y"]),
                     predator_lin_vel_x=tuple(env.command_ranges["predator_lin_vel_x"]), predator_lin_vel_y=tuple(env.command_ranges["predator_lin_vel_y"]),
                     capture_dist=float(env.capture_dist), half_fov=1.20428 / 2., max_rel_pos=float(env.MAX_REL_POS), ll_rew_weight=2.0,
                     scale_evasion_dt=float(env.reward_scales_prey["evasion"]), scale_pursuit_dt=float(env.reward_scales_pred["pursuit"]),
                     scale_termination_prey_dt=float(env.reward_scales_prey.get("termination", 0.0)), sim_dt=float(ll.cfg.sim.dt), predator_z=0.3,
                     max_episode_length_s=float(env.max_episode_length_s), base_init_state=tuple(float(v) for v in ll.base_init_state),
                     default_dof_pos=tuple(float(v) for v in ll.default_dof_pos[0]))


OUT_KEYS = ("in_command_prey", "in_command_pred", "in_root_states", "in_ll_rew", "in_ll_dones", "step", "u_root", "u_pred", "u_dof", "command_prey", "command_pred",
            "ll_commands", "predator_integrated", "predator_pos", "root_states", "dof_pos", "dof_vel", "obs_prey", "obs_pred", "rew_prey", "rew_pred", "reset_buf",
            "time_out_buf", "curr_episode_step", "episode_length_buf", "episode_sums", "sense_pos", "sense_flag", "episode_means")
STATE_KEYS = ("predator_pos", "obs_prey", "dof_pos", "dof_vel", "curr_episode_step", "episode_length_buf", "episode_sums", "episode_means")


def sequence(tag, calls, seed, rng, tweak=None):
    import torch
    origins = mgg.grid_origins(N)
    env, ll, draws = build_objects(tweak)
    ll.env_origins = torch.from_numpy(origins).clone()
    p = twin_params(env, ll, seed)
    L = p["max_episode_length"]
    pred0 = (origins + np.stack((rng.uniform(-2, 2, N), rng.uniform(-2, 2, N), np.full(N, 0.3)), axis=1)).astype(F)
    ep_len = rng.integers(1, 50, N).astype(np.int64)
    late = rng.choice(np.arange(1, N), 48, replace=False)                   # time-outs: (length + 1) > L for the starts L and L + 1, and one call later for L - 1
    ep_len[late] = L - 1 + (np.arange(48) % 3)
    obs0 = np.full((N, 16), 100.0, F)
    obs0[:, 12:16] = 0                                                       # as after construction (:127-128)
    joints0 = (np.asarray(p["default_dof_pos"], F)[None, :] * (0.75 + 0.0625 * (np.arange(N)[:, None] % 9))).astype(F)     # (patterns, not noise: they compress)
    state = dict(predator_pos=pred0, obs_prey=obs0, dof_pos=joints0, dof_vel=(0.125 * ((np.arange(N)[:, None] + np.arange(dt.NUM_DOF)[None, :]) % 7 - 3)).astype(F),
                 curr_episode_step=rng.integers(0, 50, N).astype(np.int64), episode_length_buf=ep_len, episode_sums=np.zeros((3, N), F),
                 episode_means=np.zeros(3, F), env_origins=origins)
    ll.root_states[ll.predator_indices, :3] = torch.from_numpy(pred0)
    ll.dof_pos[:] = torch.from_numpy(state["dof_pos"]); ll.dof_vel[:] = torch.from_numpy(state["dof_vel"])
    env.obs_buf_prey = torch.from_numpy(obs0).clone()
    env.obs_buf_pred = 100. * torch.ones(N, 3)
    env.rew_buf_prey, env.rew_buf_pred, env.reset_buf = torch.zeros(N), torch.zeros(N), torch.ones(N, dtype=torch.long)
    env.time_out_buf = torch.zeros(N, dtype=torch.bool)
    env.curr_episode_step = torch.from_numpy(state["curr_episode_step"]).clone()
    env.episode_length_buf = torch.from_numpy(ep_len).clone()
    env._update_agent_states()
    rec = {k: [] for k in OUT_KEYS}
    ll.feed = {"root_states": [], "ll_rew": [], "ll_dones": []}
    inner_integrate, inner_sense = type(env).step_predator_single_integrator, type(env).prey_sense_predator
    tap = {}

    def step_predator_single_integrator(self, command=None):
        inner_integrate(self, command=command)
        tap["predator_integrated"] = self.predator_pos.clone().numpy()

    def prey_sense_predator(self):
        pos, flag = inner_sense(self)
        tap["sense_pos"], tap["sense_flag"] = pos.clone().numpy(), flag[:, 0].clone().numpy()
        return pos, flag
    type(env).step_predator_single_integrator, type(env).prey_sense_predator = step_predator_single_integrator, prey_sense_predator

    def draw_commands(n):
        cp = rng.uniform(-3.0, 3.0, (n, 4)).astype(F)
        cp[:, 2] = rng.uniform(-9.0, 9.0, n)                                # beyond +-pi: the wrap of column 2
        return cp, rng.uniform(-3.0, 3.0, (n, 2)).astype(F)

    twin_state = dict(state)
    for k in range(calls):
        cmd_prey, cmd_pred = draw_commands(N)
        c_prey, c_pred, _ = dt.pre(p, cmd_prey, cmd_pred)
        pred_after = dt.integrate_predator(p, twin_state["predator_pos"], c_pred)
        root, ll_rew, ll_dones = mgg.draw_inputs(rng, np.arange(N), pred_after, origins, None)
        ll_dones[0] = False
        for attempt in range(40):
            step_key = 1000 * (k + 1) + attempt
            for _ in range(30):
                s = dict(twin_state, command_pred=c_pred, root_states=root, ll_rew=ll_rew, ll_reset=ll_dones)
                out, info = dt.post(p, s, step=step_key)
                viol = mgg.per_env_violations(p, info)
                viol[0] |= bool(info["visible"][0]) or bool(out["reset_buf"][0])        # env 0 stays occluded and alive: see the module docstring
                bad = np.nonzero(viol)[0]
                if len(bad) == 0:
                    break
                cmd_prey[bad], cmd_pred[bad] = draw_commands(len(bad))                    # (the predator's own position margin depends on its velocity)
                c_prey, c_pred, _ = dt.pre(p, cmd_prey, cmd_pred)
                pred_after = dt.integrate_predator(p, twin_state["predator_pos"], c_pred)
                r2, w2, d2 = mgg.draw_inputs(rng, bad, pred_after, origins, None)
                root[bad], ll_rew[bad], ll_dones[bad] = r2, w2, d2
                ll_dones[0] = False
            if len(bad) == 0:
                break
        assert len(bad) == 0, "could not clear the threshold margins"
        dt.assert_margins(p, info)
        ll.call = k
        ll.feed["root_states"].append(torch.from_numpy(root).clone())
        ll.feed["ll_rew"].append(torch.from_numpy(ll_rew).clone())
        ll.feed["ll_dones"].append(torch.from_numpy(ll_dones).clone())
        done_ids = np.nonzero(out["reset_buf"])[0]
        draws.begin(seed, step_key, done_ids, False)
        prey_t, pred_t = torch.from_numpy(cmd_prey).clone(), torch.from_numpy(cmd_pred).clone()
        with mgg._patched_torch(draws):
            obs_pred, obs_prey, _, _, rew_pred, rew_prey, reset_buf, extras = env.step(pred_t, prey_t)      # the reference's own step(), whole
        assert np.array_equal(np.nonzero(reset_buf.numpy())[0], done_ids), "twin and reference disagree on the done envs"
        u_root, u_pred, u_dof = dt.draws(seed, N, step_key)
        means = np.array([float(extras["episode"]["rew_prey_evasion"]), float(extras["episode"]["rew_pred_pursuit"]),
                          float(extras["episode"].get("rew_prey_termination", 0.0))], F)
        sums = np.stack([env.episode_sums_prey["evasion"].clone().numpy(), env.episode_sums_pred["pursuit"].clone().numpy(),
                         env.episode_sums_prey["termination"].clone().numpy() if "termination" in env.episode_sums_prey else np.zeros(N, F)])
        vals = dict(in_command_prey=cmd_prey, in_command_pred=cmd_pred, in_root_states=root.copy(), in_ll_rew=ll_rew.copy(), in_ll_dones=ll_dones.copy(), step=step_key,
                    u_root=u_root, u_pred=u_pred, u_dof=u_dof, command_prey=prey_t.numpy().copy(), command_pred=pred_t.numpy().copy(),
                    ll_commands=ll.commands.clone().numpy(), predator_integrated=tap["predator_integrated"], predator_pos=env.predator_pos.clone().numpy(),
                    root_states=ll.root_states[ll.prey_indices].clone().numpy(), dof_pos=ll.dof_pos.clone().numpy(), dof_vel=ll.dof_vel.clone().numpy(),
                    obs_prey=obs_prey.clone().numpy(), obs_pred=obs_pred.clone().numpy(), rew_prey=rew_prey.clone().numpy(), rew_pred=rew_pred.clone().numpy(),
                    reset_buf=reset_buf.clone().numpy(), time_out_buf=extras["time_outs"].clone().numpy(), curr_episode_step=env.curr_episode_step.clone().numpy(),
                    episode_length_buf=env.episode_length_buf.clone().numpy(), episode_sums=sums, sense_pos=tap["sense_pos"], sense_flag=tap["sense_flag"],
                    episode_means=means)
        for name in OUT_KEYS:
            rec[name].append(vals[name])
        twin_state = {kk: out[kk] for kk in STATE_KEYS + ("env_origins",)}
        cap, to = info["capture"], info["time_out"]
        print(f"  {tag} call {k}: step key {step_key}, visible {int(tap['sense_flag'].sum())}/{N}, captured {int(cap.sum())}, timed out {int(to.sum())}, "
              f"ll only {int((ll_dones & ~cap & ~to).sum())}, neither {int((~out['reset_buf']).sum())}, means {means}")
    res = {f"{tag}_{k}": np.stack(v) if k != "step" else np.array(v, np.int64) for k, v in rec.items()}
    res.update({f"{tag}_in0_{k}": state[k] for k in STATE_KEYS})
    res[f"{tag}_env_origins"] = origins
    res[f"{tag}_params"] = np.array(json.dumps(p))
    return res


def _with_termination(cfg):
    cfg.rewards_prey.scales.termination = -25.0


def step_fixture():
    mg.EXECUTED.clear()
    rng = np.random.default_rng(40)
    out = {}
    out.update(sequence("a", 4, seed=21, rng=rng))
    out.update(sequence("t", 2, seed=22, rng=rng, tweak=_with_termination))
    out["base_quat_source"] = np.array("root_states at read time (after the step's resets)")
    out["env0"] = np.array("occluded and not done in every call")
    np.savez_compressed(os.path.join(mg.OUT, "dec_game_step.npz"), **out)
    record_provenance("dec_game_step.npz")
    print("dec_game_step.npz written")


if __name__ == "__main__":
    which = sys.argv[1:] or ["configs", "step"]
    for w in which:
        {"configs": configs, "step": step_fixture}[w]()
