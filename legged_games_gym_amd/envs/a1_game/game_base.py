"""What ``HighLevelGame`` and ``DecHighLevelGame`` share: the device choice, the low-level ``a1`` env with its frozen locomotion policy, the
common part of the configs, parameter struct and pointer table, root-state resets and predator placement, the outcome statistics, the
reference-named state views and the capture hooks the runner's device rollout touches."""
import copy
import os
import types

import numpy as np
import torch

from legged_games_gym_amd import capi
from legged_games_gym_amd.envs.base.base_task import parse_device_str
from legged_games_gym_amd.utils.helpers import class_to_dict, get_load_path, parse_sim_params

HALF_FOV = 1.20428 / 2.0        # high_level_game.py:427, dec_high_level_game.py:417
LL_REW_WEIGHT = 2.0             # high_level_game.py:364, dec_high_level_game.py:328
PREDATOR_Z = 0.3                # low_level_game.py:432


class GameBase:
    TASK = "high_level_game"    # the task's name in error messages
    GRAPHED_ACTORS = "a FusedActor"                  # whom make_graphed_policy_step's step-counter check names
    # outcome statistics of the task: the names of the counts and of the means, the buffers constructor, whether the struct has a reduction
    # ``ticket``, and whether ``extras["episode"]`` holds nothing but the outcomes (it then goes with them when they are switched off)
    OUTCOME_COUNTS, OUTCOME_MEANS, OUTCOME_BUFFERS = capi.OUTCOME_COUNTS, capi.OUTCOME_MEANS, staticmethod(capi.outcome_buffers)
    OUTCOME_TICKET = OUTCOME_ONLY_EPISODE = True

    def _init_low_level(self, cfg, sim_params, physics_engine, sim_device, headless, root_dir):
        """The reference constructor up to and including the low-level policy (high_level_game.py:41-103, dec_high_level_game.py:41-103).
        ``root_dir`` is where ``logs/<a1 experiment>`` is searched for the low-level checkpoint when ``env.ll_policy_path`` is None."""
        from legged_games_gym_amd.envs import task_registry, LeggedRobot
        from legged_games_gym_amd.rl import ActorCritic, FusedActor
        self.cfg = cfg
        self.sim_params = sim_params
        self.height_samples = None
        self.debug_viz = False
        self.init_done = False
        self.physics_engine = physics_engine
        self.sim_device = sim_device
        sim_device_type, self.sim_device_id = parse_device_str(self.sim_device)
        self.headless = headless
        self.capture_dist = self.cfg.env.capture_dist
        self.MAX_REL_POS = 100.
        if sim_device_type in ("cuda", "gpu") and getattr(sim_params, "use_gpu_pipeline", True):
            self.device = f"cuda:{self.sim_device_id}"
        else:
            self.device = "cpu"
        self.graphics_device_id = -1 if headless else self.sim_device_id

        # low-level env: a DEEP COPY of the registered a1 configs with the overrides of :70-85 (the reference mutates the registered objects)
        ll_env_cfg, ll_train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(name="a1"))
        ll_env_cfg.env.num_envs = self.cfg.env.num_envs
        ll_env_cfg.terrain.num_rows = self.cfg.terrain.num_rows
        ll_env_cfg.terrain.num_cols = self.cfg.terrain.num_cols
        ll_env_cfg.terrain.curriculum = self.cfg.terrain.curriculum
        ll_env_cfg.noise.add_noise = self.cfg.noise.add_noise
        ll_env_cfg.domain_rand.randomize_friction = self.cfg.domain_rand.randomize_friction
        ll_env_cfg.domain_rand.push_robots = self.cfg.domain_rand.push_robots
        ll_env_cfg.terrain.mesh_type = self.cfg.terrain.mesh_type
        ll_env_cfg.rewards.scales.torques = -5.        # "instantaneous control effort cost" (:83-85)
        ll_env_cfg.seed = getattr(self.cfg, "seed", ll_env_cfg.seed)
        ll_args = types.SimpleNamespace(use_gpu=True, subscenes=0, num_threads=0, use_gpu_pipeline=getattr(sim_params, "use_gpu_pipeline", True))
        ll_sim_params = parse_sim_params(ll_args, {"sim": class_to_dict(ll_env_cfg.sim)})
        self.ll_env = LeggedRobot(cfg=ll_env_cfg, sim_params=ll_sim_params, physics_engine=physics_engine, sim_device=sim_device, headless=headless)
        ll = self.ll_env

        # frozen low-level policy: the checkpoint's actor on the MFMA actor kernel
        path = getattr(self.cfg.env, "ll_policy_path", None)
        if path is None:
            log_root = os.path.join(root_dir, "logs", ll_train_cfg.runner.experiment_name)
            try:
                path = get_load_path(log_root, load_run=ll_train_cfg.runner.load_run, checkpoint=ll_train_cfg.runner.checkpoint)
            except (ValueError, IndexError, OSError) as exc:
                raise RuntimeError(
                    f"{self.TASK} needs a trained low-level policy and found no a1 checkpoint under {log_root} ({exc}). Train the a1 task first "
                    "(python -m legged_games_gym_amd.scripts.train --task=a1 --headless) or set env.ll_policy_path to a model_*.pt file.") from exc
        if not os.path.isfile(path):
            raise RuntimeError(f"{self.TASK}: low-level checkpoint {path} does not exist. Train the a1 task first "
                               "(python -m legged_games_gym_amd.scripts.train --task=a1 --headless) or set env.ll_policy_path to a model_*.pt file.")
        self.ll_policy_path = path
        num_critic_obs = ll.num_privileged_obs if ll.num_privileged_obs is not None else ll.num_obs
        self._ll_actor_critic = ActorCritic(ll.num_obs, num_critic_obs, ll.num_actions, **class_to_dict(ll_train_cfg.policy)).to(self.device)
        self._ll_actor_critic.load_state_dict(torch.load(path, map_location=self.device, weights_only=True)["model_state_dict"])
        self._ll_actor_critic.eval()
        self._ll_fused = FusedActor(self._ll_actor_critic, self.device, seed=int(getattr(ll_env_cfg, "seed", 1)))
        self.ll_policy = self._ll_fused.act_inference

    def _parse_cfg(self, cfg):
        """The part of the reference's ``_parse_cfg`` both games state (high_level_game.py:563-571, dec_high_level_game.py:581-590)."""
        self.command_ranges = class_to_dict(self.cfg.commands.ranges)
        if self.cfg.terrain.mesh_type not in ["heightfield", "trimesh"]:
            self.cfg.terrain.curriculum = False
        self.max_episode_length_s = self.cfg.env.episode_length_s
        self.max_episode_length = np.ceil(self.max_episode_length_s / self.ll_env.dt)

    def _pack_common(self, P):
        """The fields ``lg_game_params`` and ``lg_dec_game_params`` share, from the configs."""
        ll = self.ll_env
        P.num_envs, P.decimation = self.num_envs, int(ll.cfg.control.decimation)
        P.heading_command, P.custom_origins = int(bool(self.cfg.commands.heading_command)), int(bool(ll.custom_origins))
        seed = getattr(self.cfg, "seed", 1)
        P.seed = int(seed) if seed is not None and seed >= 0 else 1
        for name, key in (("cmd_lin_vel_x", "lin_vel_x"), ("cmd_lin_vel_y", "lin_vel_y"), ("predator_lin_vel_x", "predator_lin_vel_x"),
                          ("predator_lin_vel_y", "predator_lin_vel_y")):
            capi._fill(getattr(P, name), self.command_ranges[key])
        P.capture_dist = float(self.capture_dist)
        P.half_fov, P.max_rel_pos, P.ll_rew_weight = HALF_FOV, self.MAX_REL_POS, LL_REW_WEIGHT
        P.sim_dt, P.predator_z = float(ll.cfg.sim.dt), PREDATOR_Z
        capi._fill(P.base_init_state, ll.base_init_state.cpu().numpy())

    def _ll_pointers(self):
        """The low-level sim's buffers that both games' pointer tables name."""
        b = self.ll_env._sim.buf
        return {"ll_" + name: b[name].data_ptr() for name in ("root_states", "commands", "env_origins", "rew_buf", "reset_buf", "step_counter")}

    def _own(self, command, width, scratch, name):
        """``command`` where the kernels can read and clip it: the caller's tensor, or its copy in ``scratch`` when that one is not a contiguous
        float32 tensor on this device."""
        if command.shape != (self.num_envs, width):
            raise ValueError(f"{name} must be [{self.num_envs},{width}], got {tuple(command.shape)}")
        if command.dtype != torch.float32 or not command.is_contiguous() or str(command.device) != str(self.device):
            scratch.copy_(command)
            command = scratch
        return command

    def _reset_roots(self, ids):
        """The root-state part of ``reset_idx`` (high_level_game.py:326-349, dec_high_level_game.py:271-311): the prey at its env origin
        with a random velocity, then the predator placed around it."""
        ll, n = self.ll_env, len(ids)
        root = ll.base_init_state.repeat(n, 1)
        root[:, :3] += ll.env_origins[ids]
        if ll.custom_origins:
            root[:, :2] += 2.0 * torch.rand(n, 2, device=self.device) - 1.0
        root[:, 7:13] = torch.rand(n, 6, device=self.device) - 0.5
        ll.root_states[ids] = root
        self.predator_pos[ids] = self._place_predator(root[:, :3])

    def _require_device_step_counter(self, fused):
        if fused.step_counter is None or fused.step_counter.data_ptr() != self.ll_env._sim.buf["step_counter"].data_ptr():
            raise ValueError(f"make_graphed_policy_step needs {self.GRAPHED_ACTORS} on the low-level sim's device step counter")

    def _fill_optional_outputs(self, out, n, command, mean, std, obs_in):
        """The optional outputs of an actor launch (``sample`` / ``sigma`` / ``log_prob`` / ``obs_copy`` in ``out``, absent or None when not
        asked for), written from the host when the launch had no shared kernel (rc -4)."""
        if out.get("sample") is not None:
            out["sample"].view(n, -1).copy_(command)
        if out.get("sigma") is not None:
            out["sigma"].view(n, -1).copy_(std.expand(n, -1))
        if out.get("log_prob") is not None:
            out["log_prob"].view(n).copy_(torch.distributions.Normal(mean, std).log_prob(command).sum(-1))
        if out.get("obs_copy") is not None:
            out["obs_copy"].view(n, -1).copy_(obs_in)

    # ------------------------------------------------------------------ whether a shared recurrent launch is available
    # What both envs' deciders are made of; each env keeps the order of its checks and the text of its message (``_say_separate``).
    def _load_or_say(self, load, say, *said_for):
        """``load()``, a ``capi.load_*_library``; None, with the env's one-line message, for a build without the library."""
        try:
            return load()
        except (RuntimeError, OSError) as exc:
            self._say_separate(f"{type(exc).__name__}: {exc}", say, *said_for)
            return None

    @staticmethod
    def _wide_precision_0(fused):
        """The low-level role of a shared recurrent launch is the split-bf16 kernel: wide precision 0 takes the separate actor launches.
        Asked per call: ``lg_mlp_wide_set_precision`` may change between calls (an invalid mode changes nothing and returns the current one)."""
        return fused.lib.lg_mlp_wide_set_precision(-1) != 1

    def _say_once(self, key, say, line):
        said = self.__dict__.setdefault("_separate_said", set())
        if say and key not in said:
            said.add(key)
            print(line)

    # ------------------------------------------------------------------ outcome statistics
    def enable_outcome_stats(self, on=True):
        """Switch the outcome statistics on or off.  On: ``_post`` issues the outcome entry point of the task on every step path and
        ``extras["episode"]`` holds a 0-dim view ``outcome_<name>`` per name in ``OUTCOME_MEANS``: shares of the done envs of the last step
        in which an env was done (an env may raise several), and ``outcome_steps``, their mean episode length in high-level steps.  Off: the
        launches and the extras of the plain task (``extras == {}`` for ``HighLevelGame``).  The totals are kept across a switch;
        ``reset_outcome_totals()`` zeroes them.

        A graph captures the launch that the switch selected at capture time: flip the switch BEFORE ``make_graphed_step``,
        ``make_graphed_policy_step`` or the runner's device rollout capture; a graph captured earlier keeps replaying what it captured."""
        if self.OUTCOME_ONLY_EPISODE:
            self.extras.pop("episode", None)
        else:
            for key in [k for k in self.extras["episode"] if k.startswith("outcome_")]:
                del self.extras["episode"][key]
        if not on:
            self._outcome = None
            return
        if getattr(self, "_outcome_accum", None) is None:
            dev = self.device
            self._outcome_accum = torch.zeros(len(self.OUTCOME_COUNTS), device=dev, dtype=torch.int64)
            if self.OUTCOME_TICKET:
                self._outcome_ticket = torch.zeros(1, device=dev, dtype=torch.int32)
            self._outcome_means = torch.zeros(len(self.OUTCOME_MEANS), device=dev, dtype=torch.float)
            self._outcome_totals = torch.zeros(len(self.OUTCOME_COUNTS), device=dev, dtype=torch.int64)
        pointers = {"ll_time_out_buf": self.ll_env._sim.buf["time_out_buf"].data_ptr(), "accum": self._outcome_accum.data_ptr(),
                    "means": self._outcome_means.data_ptr(), "totals": self._outcome_totals.data_ptr()}
        if self.OUTCOME_TICKET:
            pointers["ticket"] = self._outcome_ticket.data_ptr()
        self._outcome = self.OUTCOME_BUFFERS(pointers)
        self.extras.setdefault("episode", {}).update({f"outcome_{name}": self._outcome_means[i] for i, name in enumerate(self.OUTCOME_MEANS)})

    def outcome_totals(self):
        """Running sums since construction or the last ``reset_outcome_totals()``, as Python ints after ONE synchronising copy, under the
        names of ``OUTCOME_COUNTS``.  Episodes still running are not in them."""
        if getattr(self, "_outcome_totals", None) is None:
            raise RuntimeError("the outcome statistics were never switched on: enable_outcome_stats() or env.outcome_stats = True")
        return dict(zip(self.OUTCOME_COUNTS, (int(v) for v in self._outcome_totals.cpu().tolist())))

    def reset_outcome_totals(self):
        """Zero the totals on the current stream (no synchronisation)."""
        if getattr(self, "_outcome_totals", None) is None:
            raise RuntimeError("the outcome statistics were never switched on: enable_outcome_stats() or env.outcome_stats = True")
        self._outcome_totals.zero_()

    def _check_output(self, name, t, numel):
        """An optional output of ``_act``: None, or a contiguous float32 tensor on this device with ``numel`` elements."""
        if t is None:
            return
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != numel or str(t.device) != str(self.device):
            raise ValueError(f"{name} must be a contiguous float32 tensor with {numel} elements on {self.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")

    # ------------------------------------------------------------------ graph capture of a step
    def _capture(self, device_step, warmup, steps_per_replay, result):
        """Warm up on a side stream, capture ``steps_per_replay`` x ``device_step`` into one HIP graph, return the replay callable
        returning ``result()`` -- no host between the launches (same contract as ``LeggedRobot.make_graphed_step``)."""
        ll = self.ll_env
        sim = ll._sim
        sim.set_obs_output(ll.obs_buf)                       # one fixed low-level observation buffer while replaying
        sim.buf["step_counter"].fill_(ll.common_step_counter)
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            for _ in range(warmup):
                device_step()
                ll.common_step_counter += 1
        torch.cuda.current_stream(self.device).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        ll.begin_graph_capture()
        sim.set_deferred_extras(False)                       # the low-level step publishes its extras in its own launch
        try:
            with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                for _ in range(steps_per_replay):
                    device_step()
        finally:
            ll.end_graph_capture(0)                          # (the captured steps went through the sim, not through ll_env.step)

        def replay():
            graph.replay()
            ll.common_step_counter += steps_per_replay
            return result()
        return graph, replay

    # ------------------------------------------------------------------ capture hooks of the runner's device rollout
    @property
    def _capturing(self):
        return self.ll_env._capturing

    @property
    def common_step_counter(self):
        return self.ll_env.common_step_counter

    @common_step_counter.setter
    def common_step_counter(self, value):
        self.ll_env.common_step_counter = value

    def begin_graph_capture(self):
        """Several ``step_policy`` calls are about to be captured into one HIP graph: the step counter moves to the device."""
        self.ll_env.begin_graph_capture()

    def capture_extras_flush(self):
        self.ll_env.capture_extras_flush()

    def end_graph_capture(self, steps_captured: int):
        self.ll_env.end_graph_capture(steps_captured)

    def capture_state(self):
        """``LeggedRobot.capture_state`` of the game: its own observation ping-pong and the low-level env's state (flip and counter)."""
        return self._obs_flip, self.ll_env.capture_state()

    def abort_graph_capture(self, state):
        """``LeggedRobot.abort_graph_capture`` of the game: the env's own buffers back on ``state``'s side of their pairs; the low-level env
        leaves capture mode and restores its flip, the sim's output binding and the counter."""
        self._obs_flip, ll_state = state
        self._select_observations()
        self.ll_env.abort_graph_capture(ll_state)

    def render(self, sync_frame_time=True):
        return None     # headless

    # ------------------------------------------------------------------ state views (reference names)
    @property
    def prey_states(self):
        return self.ll_env.root_states

    @property
    def base_quat(self):
        return self.ll_env.root_states[:, 3:7]

    @property
    def dt(self):
        return self.ll_env.dt

    # ------------------------------------------------------------------ set-up
    def _place_predator(self, prey_pos):
        """low_level_game.py:420-432: a common sign per env times U(1, 10) on every axis, then z = 0.3."""
        n = prey_pos.shape[0]
        offset = 1.0 + 9.0 * torch.rand(n, 3, device=self.device)
        sign = torch.where(torch.rand(n, 1, device=self.device) < 0.5, -1.0, 1.0)
        pos = prey_pos - sign * offset
        pos[:, 2] = PREDATOR_Z
        return pos
