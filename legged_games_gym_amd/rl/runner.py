"""``OnPolicyRunner`` with the constructor / learn / save / load / get_inference_policy surface the
reference uses (``task_registry.py:154-161``, ``scripts/train.py:43``, ``scripts/play.py:59``);
checkpoints are ``model_<it>.pt`` in ``log_dir`` so ``get_load_path`` (helpers.py:103-125) finds them."""
import os
import statistics
import time
from collections import deque

import torch

from .. import capi
from .actor_critic import ActorCritic, ActorCriticRecurrent
from .ppo import PPO


def critic_input_width(state_dict):
    """The input width of the critic in an ``ActorCritic`` / ``ActorCriticRecurrent`` state dict: of the critic memory where there is one, of
    the critic MLP's first layer otherwise; None when it has neither."""
    for key in ("memory_c.rnn.weight_ih_l0", "critic.0.weight"):
        if key in state_dict:
            return int(state_dict[key].shape[1])
    return None


def check_critic_width(actor_critic, state_dict, agent=None):
    """Refuse a checkpoint whose critic reads another number of inputs than ``actor_critic`` 's with an error that names the switch, instead of
    ``load_state_dict`` 's size-mismatch trace: the privileged critic of dec_high_level_game (``--privileged_critic {prey,pred,both}``)."""
    have, want = critic_input_width(state_dict), critic_input_width(actor_critic.state_dict())
    if have is not None and want is not None and have != want:
        who = f"the {agent} agent's " if agent else "the "
        raise ValueError(f"{who}checkpoint has a critic with {have} inputs, this runner's critic has {want}: the critic's input width follows the privileged "
                         "observations, so run with the --privileged_critic {prey,pred,both} the checkpoint was trained with (or without it)")


class OnPolicyRunner:
    _csv = _csv_cols = None                 # progress.csv and its columns, opened with the writer (_log_scalars)

    def __init__(self, env, train_cfg, log_dir=None, device="cpu"):
        self.cfg, self.alg_cfg, self.policy_cfg = train_cfg["runner"], train_cfg["algorithm"], train_cfg["policy"]
        self.device, self.env = device, env
        num_critic_obs = env.num_privileged_obs if env.num_privileged_obs is not None else env.num_obs
        name = self.cfg.get("policy_class_name", "ActorCritic")
        classes = {"ActorCritic": ActorCritic, "ActorCriticRecurrent": ActorCriticRecurrent}
        if name not in classes:
            raise NotImplementedError(f"policy class {name!r} is not bundled (available: {', '.join(classes)})")
        actor_critic = classes[name](env.num_obs, num_critic_obs, env.num_actions, **self.policy_cfg).to(device)
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            for prm in actor_critic.parameters():       # replicas start from rank 0's weights (env seeds differ per rank)
                dist.broadcast(prm.data, src=0)
        self.alg = PPO(actor_critic, device=device, device_bptt=self.cfg.get("device_bptt", False), **self.alg_cfg)      # (device_bptt: a runner key like device_rollout, not a config field)
        self.num_steps_per_env = self.cfg["num_steps_per_env"]
        self.save_interval = self.cfg["save_interval"]
        self.alg.init_storage(env.num_envs, self.num_steps_per_env, [env.num_obs], [env.num_privileged_obs], [env.num_actions])
        self.log_dir, self.writer = log_dir, None
        self.tot_timesteps, self.tot_time, self.current_learning_iteration = 0, 0.0, 0
        _, _ = self.env.reset()
        self._fused = self._make_fused_actor()

    def _init_rollout_state(self):
        """Everything the rollouts keep between calls, with its "not yet" value: the generic loop, no device actor."""
        self._fused = None                  # the device actor: a FusedActor or a RecurrentFusedActor
        self._game_rollout = False          # the device rollout goes through env.step_policy of a game task (else: a locomotion env)
        self._recurrent_rollout = False     # ... with the memories of a recurrent policy on the device
        self._fused_step = None             # locomotion: lg_step_policy (True) or actor kernel + lg_step (False); None until the first rollout decides
        self._rolled = None                 # ... or the whole rollout in one launch (lg_rollout_policy), decided likewise
        self._roll = None                   # the storage lg_rollout_policy writes
        self._time_outs = None              # [T, N, 1] time-out floats of the rollout (locomotion, an agent view of dec_high_level_game)
        self._critic_features = None        # [T, N, H] the critic memory's output of every step (recurrent)
        self._priv_carry = None             # [N, P] the privileged rows behind the rollout's last step (an agent view with privileged observations)
        self._critic_fwd = None             # _critic_values: the learner kernels' forward of the critic (False: torch)
        self._critic_chunks = self._critic_out = None     # ... in row chunks, and where their values are gathered

    def use_generic_loop(self):
        """Drop the device actor and its mode: the rollouts take the generic VecEnv loop."""
        self._init_rollout_state()

    def _make_fused_actor(self):
        """Rollouts with the MFMA actor (and, for the flat task, the actor fused into the step kernel) instead of torch ops;
        the critic, log-probs and the time-out bootstrap are then evaluated once per rollout on all T x N transitions.  Decides the mode:
        the generic loop (None), the device rollout of a locomotion env or of a game task (``device_rollout``, opt-in: ``high_level_game``,
        ``scripted_predator_game``, an agent view of ``dec_high_level_game``), each feed-forward or recurrent.

        Recurrent policy: both memories in one ``lg_lstm_step`` launch, then the MFMA actor on the actor memory's output, per step
        (``RecurrentFusedActor``); the critic MLP once per rollout on the critic memory's outputs of all T steps.  A memory the device cell
        does not cover (a GRU without the key ``device_gru``, several layers, more than 256 units without ``wide_memory``) takes the torch
        loop.  On a game task the same actor goes through ``env.step_policy`` (lg_lstm_step -> lg_game_lstm_act -> lg_step -> post)."""
        self._init_rollout_state()
        env, cfg = self.env, self.cfg
        alg = getattr(self, "alg", None)              # (tests/test_game_policy_abi.py calls this on a bare runner that has no learner yet)
        ac = alg.actor_critic if alg is not None else None
        rec = ac is not None and ac.is_recurrent
        cuda, game = str(self.device).startswith("cuda"), hasattr(env, "ll_env")
        view = getattr(env, "dec_agent_view", False)  # (its critic may read privileged observations, and it sends time-outs)
        priv = env.num_privileged_obs is not None
        unserved = priv and not view                  # privileged observations the device rollouts have no critic path for
        why, hint, more = None, "", {}
        if game:
            if not cfg.get("device_rollout", False):
                return None
            if not cuda:
                why = f"the policy is on {self.device}, the game actor kernels run on a GPU"
            elif not hasattr(env, "step_policy"):
                why = "the game actor kernels have no recurrent policy for this task"
            elif unserved:
                why = "privileged observations"
            if why is not None and not rec:               # (a feed-forward policy never said why)
                return None
        elif not (cuda and cfg.get("fused_rollout", True) and hasattr(env, "_sim")) or (unserved and not rec):
            return None
        if rec and why is None:
            wide = bool(cfg.get("wide_memory", False))    # opt-in: memories of up to 512 units on liblegged_lstm_wide.so
            gru, cell_why, hint = self._recurrent_cell_reason(ac, wide)       # opt-in: GRU memories on liblegged_gru.so (the key device_gru)
            if not game and (unserved or cell_why is not None):
                print(f"[runner] device {'GRU' if gru else 'LSTM'} cell unavailable ({'privileged observations' if unserved else cell_why}); "
                      f"torch policy in the rollout{hint}")
                return None
            if cell_why is not None:
                why = f"no device {'GRU' if gru else 'LSTM'} cell for a {cell_why}"
            else:
                hint = ""
            more = dict({"gru": True} if gru else {}, num_envs=env.num_envs, wide=wide)
            if game and gru and cfg.get("dec_gru_shared", False):
                more["shared_gru"] = True
        fused = self._build_actor(ac, game, rec, why, hint, more)
        if fused is None:
            return None
        T, N = self.num_steps_per_env, env.num_envs
        if not game or view:
            self._time_outs = torch.zeros(T, N, 1, device=self.device)
        if rec:
            self._critic_features = torch.zeros(T, N, ac.memory_c.rnn.hidden_size, device=self.device)
            self._fused_step, self._rolled = False, False         # neither lg_step_policy nor lg_rollout_policy has a recurrent kernel
        if view and priv:
            self._priv_carry = torch.zeros(N, env.num_privileged_obs, device=self.device)
        self._game_rollout, self._recurrent_rollout = game, rec
        return fused

    def _build_actor(self, ac, game, rec, why, hint, more):
        """The one place a device actor is made: on the noise stream of the sim's device step counter (a game task: the low-level sim's;
        an agent view of dec_high_level_game names its agent's seed offset).  None, with the path's fall-back message, when ``why`` says so
        already or the actor's shape has no kernel -- on a game task that shows in a first launch here, not in the first rollout."""
        env = self.env
        if why is None:
            try:
                if rec:
                    from .recurrent_actor import RecurrentFusedActor as make
                else:
                    from .fused_actor import FusedActor as make
                fused = make(ac, self.device, seed=int(getattr(env.cfg, "seed", 1)) + getattr(env, "fused_seed_offset", 7919),
                             step_counter=(env.ll_env if game else env)._sim.buf["step_counter"], **more)
                if game and rec:
                    env.shared_actor_launch(fused)            # raises the new kernel's LDS limit here, outside any capture; False = separate launches
                                                              # (an agent view has no opponent yet: DecGamePolicyRunner makes the call)
                elif game:
                    fused.act_inference(env.get_observations())   # a shape lg_policy_act refuses (rc -4)
                return fused
            except Exception as exc:
                why = f"{type(exc).__name__}: {exc}"
        if game:
            print(f"[runner] device rollout unavailable ({why}); generic VecEnv loop{hint}")
        else:                                                 # unsupported actor shape: torch rollouts
            print(f"[runner] MFMA actor unavailable ({why}); torch policy in the rollout")
        return None

    @staticmethod
    def _wide_memory_hint(ac, wide):
        """What a fall-back message adds when the key ``wide_memory`` would have kept the policy on the device."""
        from .recurrent_actor import lstm_unsupported_reason, wide_memory_would_help
        rnns = (ac.memory_a.rnn, ac.memory_c.rnn)
        if wide or not any(wide_memory_would_help(r) for r in rnns) or any(lstm_unsupported_reason(r, wide=True) for r in rnns):
            return ""
        return " (the runner key wide_memory / --wide_memory covers up to 512 units)"

    def _recurrent_cell_reason(self, ac, wide):
        """``(gru, why, hint)``: whether the key ``device_gru`` applies (it is set and both memories are ``nn.GRU``), why the device cell does
        not take the memories (None: it does) and what the fall-back message adds on the same line."""
        import torch.nn as nn
        from .recurrent_actor import device_gru_would_help, gru_unsupported_reason, lstm_unsupported_reason
        rnns = (ac.memory_a.rnn, ac.memory_c.rnn)
        if bool(self.cfg.get("device_gru", False)) and all(isinstance(r, nn.GRU) for r in rnns):
            return True, gru_unsupported_reason(rnns[0]) or gru_unsupported_reason(rnns[1]), ""
        why = lstm_unsupported_reason(rnns[0], wide) or lstm_unsupported_reason(rnns[1], wide)
        hint = self._wide_memory_hint(ac, wide)
        if why is not None and all(device_gru_would_help(r) for r in rnns):
            hint += " (the runner key device_gru / --device_gru runs GRU memories on the device)"
        return False, why, hint

    def _recurrent_last_values(self, critic_obs):
        """The value behind the rollout's last step from one critic-only ``lg_lstm_step`` into scratch outputs: the carried state stays."""
        return self.alg.actor_critic.critic(self._fused.peek_critic(critic_obs, reset=self.env.reset_buf)).detach()

    def _fused_env_step(self, obs):
        """One rollout step: ``lg_step_policy`` (actor inside the step kernel) where a fused kernel exists, else actor kernel + step."""
        env, fused = self.env, self._fused
        if self._fused_step is not False:
            try:
                (actions, mean), out = env.step_policy(fused)
                self._fused_step = True
                return actions, mean, out
            except RuntimeError as exc:
                # only "no fused kernel for this sim / actor pair" (lg_step_policy rc -4) selects the two-kernel path;
                # a real HIP failure must surface
                if self._fused_step or "fused policy step" not in str(exc):
                    raise
                self._fused_step = False
        actions, mean = fused.act_with_mean(obs)
        return actions, mean, env.step(actions)

    def _critic_values(self, st):
        """critic(obs) for all stored transitions: lg_mlp_forward / lg_mlp_wide_forward when the critic has one of the learner kernels' shapes, torch otherwise."""
        ac = self.alg.actor_critic
        cobs = (st.privileged_observations if st.privileged_observations is not None else st.observations).flatten(0, 1)
        tr = self._critic_fwd
        if tr is None or (tr is not False and (tr.inputs[0].data_ptr() != cobs.data_ptr() or tr.mb * len(self._critic_chunks or [0]) != cobs.shape[0])):
            from .mlp_kernels import MlpTrainer, WideMlpTrainer
            tr = False
            self._critic_chunks = None
            if isinstance(ac.critic, torch.nn.Sequential) and cobs.is_cuda:
                tr = MlpTrainer([ac.critic], [cobs], cobs.shape[0], forward_only=True)
                if not tr.supported:                  # the 512-256-128 critics: the chain forward of the wide learner kernels
                    # in row chunks of a mini-batch: the wide workspace is sized for TRAINING on `mb` rows (activations, gradient slabs, dW
                    # partials: 0.8 GB for all 24 x 4096 rows, 6.4 GB at 32 768 envs) although a forward needs none of the gradient regions
                    rows_all = cobs.shape[0]
                    parts = next((c for c in (4, 3, 2) if rows_all % c == 0 and rows_all // c >= 4096), 1)
                    tr = WideMlpTrainer([ac.critic], [cobs], rows_all // parts, forward_only=True)
                    if tr.supported and parts > 1:
                        self._critic_chunks = [torch.arange(i * (rows_all // parts), (i + 1) * (rows_all // parts), device=cobs.device) for i in range(parts)]
                        self._critic_out = torch.empty(rows_all, 1, device=cobs.device)
            self._critic_fwd = tr
        if tr is not False and tr.supported:
            tr.refresh()                              # parameter addresses (stable; the values follow the optimiser)
            if self._critic_chunks:
                n = self._critic_chunks[0].numel()
                for i, rows in enumerate(self._critic_chunks):
                    self._critic_out[i * n:(i + 1) * n].copy_(tr.forward(rows)[0])
                return self._critic_out
            return tr.forward(None)[0]
        return ac.evaluate(cobs)

    def _rollout_steps_rolled(self, stats):
        """The whole rollout of an iteration as ONE launch (``lg_rollout_policy``: the multi-step kernel writes observations, actions,
        means, rewards and dones straight into the PPO storage) plus ONE bookkeeping launch (``lg_rollout_finish``: sigma, log-probs,
        time-out floats, episode statistics).  Returns None when the sim / actor pair has no multi-step kernel."""
        env, alg, fused = self.env, self.alg, self._fused
        st, T = alg.storage, self.num_steps_per_env
        N, A, dev = env.num_envs, st.actions.shape[-1], self.device
        roll = self._roll
        fresh = roll is None or roll["obs"].shape[0] != T + 1 or st.observations.data_ptr() != roll["obs"].data_ptr()
        if fresh:
            with torch.inference_mode(False):         # (rollouts run under inference_mode; env.obs_buf becomes a view of this buffer and callers feed it to autograd modules)
                obs_all = torch.empty(T + 1, N, st.observations.shape[-1], device=dev)     # [T + 1]: the kernel leaves the next observations behind the stored ones
                roll = {"obs": obs_all, "actions": st.actions, "mean": st.mu, "rew": st.rewards.view(T, N), "dones": st.dones.view(T, N),
                        "time_outs": torch.zeros(T, N, dtype=torch.uint8, device=dev)}
        try:
            env.rollout_policy(fused, T, storage=roll)
        except RuntimeError as exc:
            if "multi-step rollout kernel" not in str(exc):
                raise
            return None                               # (the storage is untouched: the per-step rollout goes on with it)
        if fresh:                                     # the storage's observations become a view of the kernel's buffer only once it has run
            st.observations = roll["obs"][:T]         # (the learner kernels read the storage through this view)
            self._roll = roll
        post = capi.lg_rollout_post()
        p = lambda x: x.data_ptr()
        post.actions, post.mean, post.rewards, post.dones, post.time_outs = p(st.actions), p(st.mu), p(st.rewards), p(st.dones), p(roll["time_outs"])
        post.std, post.sigma, post.log_prob, post.time_outs_f = p(alg.actor_critic.std), p(st.sigma), p(st.actions_log_prob), p(self._time_outs)
        post.cur_return, post.cur_length, post.sums = p(stats["cur_rew"]), p(stats["cur_len"]), p(stats["_sums"])
        post.steps, post.num_envs, post.num_actions = T, N, A
        rc = fused.lib.lg_rollout_finish(post, torch.cuda.current_stream(self.device).cuda_stream)
        if rc != 0:
            raise RuntimeError(f"lg_rollout_finish failed ({rc}): {fused.lib.lg_last_error().decode()}")
        st.step = T
        st.values.copy_(self._critic_values(st).view(T, -1, 1))
        st.rewards.add_(alg.gamma * st.values * self._time_outs)
        obs = env.obs_buf
        return obs, obs

    def _step_locomotion(self, t, obs):
        """Step ``t`` of the device rollout on a locomotion env: ``actions, mean, step result``."""
        env, fused = self.env, self._fused
        if not self._recurrent_rollout:
            return self._fused_env_step(obs)
        actions, mean, h_c = fused.act_with_mean(obs, obs, reset=env.reset_buf)       # lstm -> actor -> lg_step
        self._critic_features[t].copy_(h_c)
        return actions, mean, env.step(actions)

    def _step_game(self, t, obs):
        """Step ``t`` of the device rollout on a game task: ``env.step_policy`` (lg_game_act -> lg_step -> lg_game_post; recurrent:
        lg_lstm_step -> lg_game_lstm_act -> lg_step -> post), whose actor launch writes ``sigma[t]`` and ``actions_log_prob[t]`` of the
        unclipped sample straight into the storage.  With privileged observations (an agent view) the env's privileged launch of step
        ``t`` writes slot ``t + 1`` of the storage itself, the last step the carry buffer -- no copy launch per step."""
        st, T = self.alg.storage, self.num_steps_per_env
        more = {"with_critic_memory": True} if self._recurrent_rollout else {}
        if self._priv_carry is not None:
            more["privileged_out"] = st.privileged_observations[t + 1] if t < T - 1 else self._priv_carry
        head, out = self.env.step_policy(self._fused, sigma=st.sigma[t], log_prob=st.actions_log_prob[t], **more)
        if self._recurrent_rollout:
            self._critic_features[t].copy_(head[2])
        return head[0], head[1], out

    def _rollout_steps_device(self, stats):
        """The device rollout: per step the path's launches (``_step_locomotion`` / ``_step_game``) and one ``lg_rollout_record`` (storage
        writes and episode statistics of the transition); the critic once per rollout.  A locomotion env tries the one-launch rollout
        first.  What differs by path:
        - ``sigma`` / ``log_prob``: ``lg_rollout_record`` stores them on a locomotion env; on a game task the actor launch has (the
          reference clips the command in the caller's tensor after ``PPO.act`` took the log-prob, so ``actions[t]`` is the clipped command
          while those two belong to the unclipped sample).
        - time-outs: a locomotion env and an agent view of ``dec_high_level_game`` record them per step and bootstrap on them;
          ``high_level_game`` sends none, and a view with ``env.send_timeouts = False`` records none.
        - the critic observations of an agent view with privileged observations are ``st.privileged_observations``: one copy of the carried
          rows into slot 0, the rest by ``_step_game``.
        Returns ``(obs, critic obs)`` behind the last step."""
        env, alg, fused = self.env, self.alg, self._fused
        st, T = alg.storage, self.num_steps_per_env
        game, rec, priv = self._game_rollout, self._recurrent_rollout, self._priv_carry is not None
        bootstrap = self._time_outs is not None
        if not game and self._rolled is not False and "_sums" in stats and self.cfg.get("rolled_rollout", True):
            out = self._rollout_steps_rolled(stats)
            self._rolled = out is not None
            if out is not None:
                return out
        if priv:
            st.privileged_observations[0].copy_(env.get_privileged_observations())      # (the carry of the last rollout, or the env's own after a reset / the other agent's steps)
        obs = env.get_observations()
        lib, step = fused.lib, capi.lg_rollout_step()
        p = lambda x: x.data_ptr()
        step.num_envs, step.num_obs, step.num_actions = env.num_envs, st.observations.shape[-1], st.actions.shape[-1]
        step.cur_return, step.cur_length, step.sums = p(stats["cur_rew"]), p(stats["cur_len"]), p(stats["_sums"])
        stream = torch.cuda.current_stream(self.device).cuda_stream
        step.std = None if game else p(alg.actor_critic.std)
        if rec:
            # the state this rollout starts from, once (part of the captured work); an env whose last step ended an episode starts from
            # zeros: the cell reads the env's persistent reset_buf of the previous step instead of zeroing the buffers
            st.save_initial_hidden_states(fused.hidden_states())
            keep = (env.reset_buf == 0).view(1, -1, 1)
            for hid in st.initial_hidden_a + st.initial_hidden_c:
                hid.mul_(keep)
        take_step = self._step_game if game else self._step_locomotion
        cobs = None
        for t in range(T):
            prev_obs = obs
            actions, mean, (obs, cobs, rewards, dones, infos) = take_step(t, obs)
            touts = infos.get("time_outs") if bootstrap else None
            step.obs, step.actions, step.mean, step.rewards, step.dones = p(prev_obs), p(actions), p(mean), p(rewards), p(dones)
            step.time_outs = p(touts) if touts is not None else None
            step.storage_time_outs = p(self._time_outs[t]) if not game or touts is not None else None
            step.storage_obs, step.storage_actions, step.storage_mu = p(st.observations[t]), p(st.actions[t]), p(st.mu[t])
            step.storage_rewards, step.storage_dones = p(st.rewards[t]), p(st.dones[t])
            step.storage_sigma, step.storage_log_prob = (None, None) if game else (p(st.sigma[t]), p(st.actions_log_prob[t]))
            assert dones.element_size() == 1 and (touts is None or touts.element_size() == 1) and rewards.is_contiguous()   # bool / uint8 flags
            rc = lib.lg_rollout_record(step, stream)
            if rc != 0:
                raise RuntimeError(f"lg_rollout_record failed ({rc}): {lib.lg_last_error().decode()}")
        st.step = T
        if rec:
            st.values.copy_(alg.actor_critic.critic(self._critic_features.flatten(0, 1)).view(T, -1, 1))      # critic MLP once on the memory's outputs of all steps
            fused.publish_states(env.reset_buf)                                                              # the torch memories follow the device state
        else:
            st.values.copy_(self._critic_values(st).view(T, -1, 1))                            # critic once on all transitions
        if bootstrap:
            st.rewards.add_(alg.gamma * st.values * self._time_outs)                           # bootstrap on time-outs (PPO.process_env_step)
        return obs, (cobs if priv else obs)

    # ------------------------------------------------------------------ graphed rollout
    def _rollout_steps(self, stats):
        """num_steps_per_env x (act -> env.step -> store); episode statistics as tensor ops (no host sync)."""
        if self._fused is not None:
            return self._rollout_steps_device(stats)
        env, alg = self.env, self.alg
        obs = env.get_observations()
        pobs = env.get_privileged_observations()
        cobs = pobs if pobs is not None else obs
        for _ in range(self.num_steps_per_env):
            actions = alg.act(obs, cobs)
            obs, pobs, rewards, dones, infos = env.step(actions)
            cobs = pobs if pobs is not None else obs
            alg.process_env_step(rewards, dones, infos)
            d = dones.float()
            stats["cur_rew"] += rewards
            stats["cur_len"] += 1.0
            stats["sum_rew"] += (stats["cur_rew"] * d).sum()
            stats["sum_len"] += (stats["cur_len"] * d).sum()
            stats["count"] += d.sum()
            stats["cur_rew"] *= 1.0 - d
            stats["cur_len"] *= 1.0 - d
        return obs, cobs

    def _try_build_graphed_rollout(self):
        """Capture the whole rollout of one PPO iteration into a single HIP graph (one hipGraphLaunch per iteration
        instead of ~24 x 30 eager launches).  Needs this package's env (device step counter, ping-pong obs buffers)
        and an even number of steps so the observation buffers line up between replays."""
        env = self.env
        ok = (str(self.device).startswith("cuda") and hasattr(env, "begin_graph_capture") and self.num_steps_per_env % 2 == 0
              and self.cfg.get("graphed_rollout", True) and (hasattr(env, "_sim") or self._game_rollout))
        if not ok:
            return None
        if self.alg.actor_critic.is_recurrent and not self._recurrent_rollout:
            # torch memories in the generic loop: Memory.forward leaves its state in a new tensor every step, so a replay would start every
            # rollout from the state the warm-up left at the captured address, not from the one the previous rollout ended in
            return None
        snapshot = None
        opponent = getattr(env, "opponent", None)             # (an agent view of dec_high_level_game: the other agent's memories move in every step too)
        try:
            stats = self._new_stats()
            with torch.inference_mode():
                self._rollout_steps(stats)              # one eager warm-up rollout (allocators, lazy init); discarded
                self.alg.storage.clear()
                for v in stats.values():
                    v.zero_()
                torch.cuda.synchronize()
                snapshot = env.capture_state()
                mem_flip0 = getattr(self._fused, "_flip", None)       # (recurrent policy: the (h, c) ping-pong of its memories)
                opp_flip0 = getattr(opponent, "_flip", None)
                env.begin_graph_capture()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                    obs, cobs = self._rollout_steps(stats)
                    if hasattr(env, "capture_extras_flush"):
                        env.capture_extras_flush()          # extras["episode"] of the rollout's last step (its steps defer them)
                env.end_graph_capture(self.num_steps_per_env)
                assert env.capture_state() == snapshot
            self.alg.storage.clear()
            return graph, stats, obs, cobs
        except Exception as exc:                          # fall back to eager launches
            print(f"[runner] graphed rollout unavailable ({type(exc).__name__}: {exc}); using eager steps")
            if snapshot is not None:
                # steps issued during a capture that failed part-way were counted but never executed: the env puts its observation
                # ping-pong and step counter (push / resample / RNG phase) back where they were, the memories go back here
                env.abort_graph_capture(snapshot)
                if mem_flip0 is not None:
                    self._fused._flip = mem_flip0
                if opp_flip0 is not None:
                    opponent._flip = opp_flip0
            self.alg.storage.clear()
            return None

    def _new_stats(self, cur_rew=None, cur_len=None):
        """The episode statistics a rollout keeps on the device: running return and length per env (the caller's, or new ones), and
        ``_sums`` = {sum of finished-episode returns, of their lengths, their count} with a 0-dim view of each."""
        N, dev = self.env.num_envs, self.device
        sums = torch.zeros(3, device=dev)
        return {"cur_rew": torch.zeros(N, device=dev) if cur_rew is None else cur_rew, "cur_len": torch.zeros(N, device=dev) if cur_len is None else cur_len,
                "sum_rew": sums[0], "sum_len": sums[1], "count": sums[2], "_sums": sums}

    def learn(self, num_learning_iterations, init_at_random_ep_len=False):
        if init_at_random_ep_len:
            self.env.episode_length_buf[:] = torch.randint_like(self.env.episode_length_buf, high=int(self.env.max_episode_length))
            if hasattr(self.env, "refresh_privileged_observations"):
                self.env.refresh_privileged_observations()        # (the episode clock of dec_high_level_game's privileged rows)
        obs = self.env.get_observations()
        pobs = self.env.get_privileged_observations()
        cobs = pobs if pobs is not None else obs
        obs, cobs = obs.to(self.device), cobs.to(self.device)
        self.alg.actor_critic.train()
        rewbuffer, lenbuffer = deque(maxlen=100), deque(maxlen=100)
        cur_rew = torch.zeros(self.env.num_envs, dtype=torch.float, device=self.device)
        cur_len = torch.zeros(self.env.num_envs, dtype=torch.float, device=self.device)
        graphed = self._try_build_graphed_rollout()
        if graphed is None and self._fused is not None and (self._game_rollout or self._recurrent_rollout):
            # the game's device rollout without a graph (graphed_rollout = False, odd step count, failed capture): the same launches, eagerly
            graphed = (None, self._new_stats(cur_rew, cur_len), obs, cobs)
        last = self.current_learning_iteration + num_learning_iterations
        for it in range(self.current_learning_iteration, last):
            t0 = time.time()
            if graphed is not None:
                graph, stats, obs, cobs = graphed
                with torch.inference_mode():
                    if graph is not None:
                        graph.replay()
                        self.env.common_step_counter += self.num_steps_per_env
                        self.alg.storage.step = self.num_steps_per_env
                    else:
                        obs, cobs = self._rollout_steps(stats)
                    if self.log_dir is not None:
                        s_rew, s_len, cnt = (float(v) for v in torch.stack((stats["sum_rew"], stats["sum_len"], stats["count"])).cpu())
                        if cnt > 0:
                            rewbuffer.append(s_rew / cnt); lenbuffer.append(s_len / cnt)
                        for k in ("sum_rew", "sum_len", "count"):
                            stats[k].zero_()
                    t1 = time.time()
                    if self._recurrent_rollout:
                        self.alg.compute_returns(cobs, last_values=self._recurrent_last_values(cobs))
                    else:
                        self.alg.compute_returns(cobs)
            else:
                with torch.inference_mode():
                    for _ in range(self.num_steps_per_env):
                        actions = self.alg.act(obs, cobs)
                        obs, pobs, rewards, dones, infos = self.env.step(actions)
                        cobs = pobs if pobs is not None else obs
                        obs, cobs, rewards, dones = obs.to(self.device), cobs.to(self.device), rewards.to(self.device), dones.to(self.device)
                        self.alg.process_env_step(rewards, dones, infos)
                        if self.log_dir is not None:
                            cur_rew += rewards
                            cur_len += 1
                            ids = (dones > 0).nonzero(as_tuple=False)
                            rewbuffer.extend(cur_rew[ids][:, 0].cpu().numpy().tolist())
                            lenbuffer.extend(cur_len[ids][:, 0].cpu().numpy().tolist())
                            cur_rew[ids] = 0
                            cur_len[ids] = 0
                    t1 = time.time()
                    self.alg.compute_returns(cobs)
            mean_value_loss, mean_surrogate_loss = self.alg.update()
            if self._fused is not None:
                self._fused.sync_device()                     # the MFMA actor follows the optimiser (device-side repack)
            t2 = time.time()
            self.tot_timesteps += self.num_steps_per_env * self.env.num_envs
            self.tot_time += t2 - t0
            if self.log_dir is not None:
                fps = int(self.num_steps_per_env * self.env.num_envs / (t2 - t0))
                mr = statistics.mean(rewbuffer) if len(rewbuffer) else float("nan")
                ml = statistics.mean(lenbuffer) if len(lenbuffer) else float("nan")
                row = self._log_scalars(it, fps, t1 - t0, t2 - t1, mean_value_loss, mean_surrogate_loss, mr, ml)
                print(f"it {it}/{last}  steps/s {fps}  collect {t1 - t0:.3f}s  learn {t2 - t1:.3f}s  value_loss {mean_value_loss:.4f}  "
                      f"surrogate {mean_surrogate_loss:.4f}  std {row['Policy/mean_noise_std']:.3f}  "
                      f"mean_reward {mr:.3f}  mean_ep_len {ml:.1f}")
                if it % self.save_interval == 0:
                    self.save(os.path.join(self.log_dir, f"model_{it}.pt"))
        self.current_learning_iteration += num_learning_iterations
        if self.log_dir is not None:
            self.save(os.path.join(self.log_dir, f"model_{self.current_learning_iteration}.pt"))

    def _log_scalars(self, it, fps, t_collect, t_learn, value_loss, surrogate, mean_reward, mean_len):
        """Per-iteration scalars under rsl_rl's TensorBoard tag names ([EXTERNAL] OnPolicyRunner.log): always to
        ``<log_dir>/progress.csv`` (no dependency), and to a SummaryWriter when tensorboard is importable."""
        ep = (getattr(self.env, "extras", None) or {}).get("episode") or {}
        keys = sorted(ep)
        dev_keys = [k for k in keys if torch.is_tensor(ep[k])]
        # one device -> host transfer for everything that lives on the device (mean action std + the episode means)
        dev_vals = torch.stack([self.alg.actor_critic.std.detach().mean().float()] + [ep[k].detach().float().reshape(()) for k in dev_keys]).cpu().tolist()
        row = {"iteration": it, "Loss/value_function": value_loss, "Loss/surrogate": surrogate, "Loss/learning_rate": self.alg.learning_rate,
               "Policy/mean_noise_std": dev_vals[0], "Perf/total_fps": fps, "Perf/collection_time": t_collect,
               "Perf/learning_time": t_learn, "Train/mean_reward": mean_reward, "Train/mean_episode_length": mean_len,
               "total_timesteps": self.tot_timesteps}
        got = dict(zip(dev_keys, dev_vals[1:]))
        row.update({f"Episode/{k}": got[k] if k in got else float(ep[k]) for k in keys})
        if self.writer is None:
            os.makedirs(self.log_dir, exist_ok=True)
            self._csv = open(os.path.join(self.log_dir, "progress.csv"), "a", buffering=1)
            self._csv_cols = list(row)
            if self._csv.tell() == 0:
                self._csv.write(",".join(self._csv_cols) + "\n")
            try:
                from torch.utils.tensorboard import SummaryWriter
                self.writer = SummaryWriter(log_dir=self.log_dir, flush_secs=10)
            except Exception:
                self.writer = False                              # tensorboard not installed: CSV only
        self._csv.write(",".join(repr(row.get(c, "")) if not isinstance(row.get(c, ""), str) else row[c] for c in self._csv_cols) + "\n")
        if self.writer:
            for k, v in row.items():
                if k != "iteration":
                    self.writer.add_scalar(k, v, it)
        return row

    def save(self, path, infos=None):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        torch.save({"model_state_dict": self.alg.actor_critic.state_dict(),
                    "optimizer_state_dict": self.alg.optimizer.state_dict(),
                    "iter": self.current_learning_iteration, "infos": infos}, path)

    def load(self, path, load_optimizer=True):
        d = torch.load(path, map_location=self.device, weights_only=True)
        check_critic_width(self.alg.actor_critic, d["model_state_dict"], getattr(self.env, "agent", None))
        self.alg.actor_critic.load_state_dict(d["model_state_dict"])
        if load_optimizer:
            self.alg.optimizer.load_state_dict(d["optimizer_state_dict"])
            if hasattr(self.alg, "after_optimizer_load"):
                self.alg.after_optimizer_load()               # re-link the device learning rate, drop the captured update graph
        if self._fused is not None:
            self._fused.sync_device()
        self.current_learning_iteration = d["iter"]
        return d["infos"]

    def get_inference_policy(self, device=None):
        self.alg.actor_critic.eval()
        if device is not None:
            self.alg.actor_critic.to(device)
        return self.alg.actor_critic.act_inference
