"""``DecGamePolicyRunner``: predator and prey of ``dec_high_level_game`` trained in alternating "evolutions" (the reference calls
``make_dec_alg_runner(...).learn(max_num_evolutions=, num_learning_iterations=, init_at_random_ep_len=True)``,
``legged_gym/scripts/train_dec_game.py``; its runner lives in a fork of rsl_rl that is not public, so the schedule is defined here).

Two ``OnPolicyRunner`` s, one per agent view of the same env (``DecHighLevelGame.agent_view``), each with its own ``ActorCritic``, ``PPO`` and
storage -- the learner kernels and the device rollout come with them.  Evolution ``e`` trains the PREDATOR when ``e`` is even and the PREY when
odd (the argument order of the reference's ``step``) for ``num_learning_iterations`` PPO iterations; the other agent acts with its current
policy, sampling, and is not updated.  The combined ``model_<it>.pt`` and ``progress.csv`` follow the training agent's runner (``runner.save_interval``,
every logged iteration).  ``OnPolicyRunner.learn`` captures its rollout graph when it is called, i.e. at the start of every
evolution, so a graph never outlives an update of the opponent it replays; the opponent's ``FusedActor`` is repacked in place besides.

Opponent pool (runner keys ``opponent_pool_size``, default 0 = off, and ``opponent_latest_share``, default 0.5; read with ``.get()``, no
fields of the config classes; device path only).  Alternating best responses can go round in circles, so the opponent of the learning agent
may be a mixture: every agent X has an ``OpponentPool`` around its ``FusedActor``, and the OTHER agent's view plays against it -- the live X
in the share ``opponent_latest_share`` of the 32-env blocks, up to ``opponent_pool_size`` frozen earlier versions of X in the rest.  At the
START of an evolution that trains X, X's current weights are pushed into X's pool, so the pool holds strictly earlier versions than its
live member; the pool the training view plays against is then re-assigned (which block meets which member) with a generator seeded from
``(seed, evolution)`` before ``runner.learn`` captures its graph.  The opponent samples, pooled or not, and the outcome statistics stay
pooled over all opponents unless they are on together with a pool:

Outcomes per pool member and prioritised opponents.  With a pool and the outcome statistics on
(``env.outcome_stats`` / ``--outcome_stats``), the pool the training view plays against is bound with ``env.enable_member_outcomes`` before
``runner.learn`` captures its graph, so the post launch also counts the outcomes per member, and after every evolution
``<log_dir>/opponents.csv`` gets one row per member of that pool: its blocks, the six counts OF THIS EVOLUTION and the learner's win rate.
Runner key ``opponent_priority`` (a float power, default 0 = off; read with ``.get()``; ``--opponent_priority``): above 0 the non-live blocks
are dealt in proportion to ``pfsp_weights`` of the pool's running counts -- a past opponent the learner loses to gets more envs -- instead of
round-robin; it needs ``opponent_pool_size > 0`` and the outcome statistics.  With priority 0 the calls to ``assign`` are unchanged.

Recurrent policies (``policy_class_name = "ActorCriticRecurrent"``) train on the device path only: the runner key ``device_rollout`` is
required, and so are a GPU, memories the device cell covers and no feed-forward opponent pool -- there is no generic loop for two recurrent
agents, so each of these raises with its reason instead of falling back.  A step is ``lg_dec_lstm_step`` -> ``lg_dec_game_lstm_act`` -> ``lg_step`` ->
post.  The opponent samples and only its actor memory advances; the learner's critic memory advances with it.  All actor memories carry on
across evolutions; at the start of an evolution the agent that becomes the learner zeroes its CRITIC memory's state, which did not move while
it was the opponent.

Opponent pool for recurrent policies (runner key ``opponent_pool_recurrent``, default False; read with ``.get()``; ``--opponent_pool_recurrent``).
With it, ``ActorCriticRecurrent`` and ``opponent_pool_size > 0`` the two pools are ``RecurrentOpponentPool`` s over ``ActorCriticRecurrent``
copies of the agent's own shape, a step is ``lg_dec_pool_lstm_step`` -> ``lg_dec_pool_lstm_act`` -> ``lg_step`` -> post, and the evolution loop is
the one above: push at the start, seeded ``assign`` or PFSP weights, member outcomes, ``opponents.csv``, pools in the checkpoints.  A pooled
role has ONE ``(h, c)`` state, the live opponent's; ``assign`` zeroes the rows of the blocks whose member changed or was overwritten, before
``runner.learn`` captures its graph.  The key is an explicit opt-in, like every device feature: without it the
combination keeps its refusal, and the key with feed-forward policies or without a pool raises with its reason."""
import os
import re

import torch

from .runner import OnPolicyRunner, check_critic_width

AGENTS = ("pred", "prey")
OPPONENT_COLUMNS = ("evolution", "agent", "member", "pushed_at", "blocks", "episodes", "captured", "timed_out", "fell", "ll_timed_out", "steps", "learner_win_rate")


def opponent_priority_of(runner_cfg, env):
    """The runner key ``opponent_priority`` (0 when absent), refused where it cannot work: it weights the pool's members by the outcome counts
    per member, so it needs the pool and the outcome statistics."""
    priority = float(runner_cfg.get("opponent_priority", 0) or 0)
    if priority < 0:
        raise ValueError(f"opponent_priority must be >= 0, got {priority}")
    if priority > 0 and int(runner_cfg.get("opponent_pool_size", 0) or 0) <= 0:
        raise ValueError("opponent_priority > 0 needs an opponent pool: set the runner key opponent_pool_size > 0 (--opponent_pool K)")
    if priority > 0 and getattr(env, "_outcome", None) is None:
        raise ValueError("opponent_priority > 0 needs the outcome statistics: set env.outcome_stats = True (--outcome_stats); the weights come from "
                         "the outcome counts per pool member")
    return priority


class DecGamePolicyRunner:
    def __init__(self, env, train_cfg, log_dir=None, device="cpu"):
        self.env, self.cfg, self.device, self.log_dir = env, train_cfg["runner"], device, log_dir
        self.priority = opponent_priority_of(self.cfg, env)       # before anything is built
        self.recurrent = self._check_policy_class(train_cfg, device)     # before anything is built, too
        self.pool_recurrent = bool(self.cfg.get("opponent_pool_recurrent", False))
        self.views = {a: env.agent_view(a, None) for a in AGENTS}
        self.runners = {}
        for a in AGENTS:
            cfg = dict(train_cfg, runner=dict(train_cfg["runner"]))
            self.runners[a] = OnPolicyRunner(self.views[a], cfg, os.path.join(log_dir, a) if log_dir is not None else None, device=device)
        fused = {a: self.runners[a]._fused for a in AGENTS}
        device_path = all(f is not None and self.runners[a]._game_rollout for a, f in fused.items())
        for a in AGENTS:
            other = "prey" if a == "pred" else "pred"
            if device_path:
                self.views[a].opponent = fused[other]
            else:                                         # generic path for both: a view cannot mix a device learner with a torch opponent
                self.runners[a].use_generic_loop()
                self.views[a].opponent = self._sampling_policy(other)
        if self.recurrent and not device_path:                # (an actor shape the kernels refuse: the per-agent runner has said which)
            raise NotImplementedError("ActorCriticRecurrent on dec_high_level_game runs on the device rollout only and it is unavailable (see the "
                                      "[runner] message above); there is no generic loop for two recurrent agents")
        if self.recurrent:
            env.shared_actor_launch(fused["pred"], fused["prey"])     # raises the LDS limits of the recurrent kernels here, outside any capture
        self.device_path = device_path
        self.pool_size = int(self.cfg.get("opponent_pool_size", 0) or 0)
        self.latest_share = float(self.cfg.get("opponent_latest_share", 0.5))
        self.seed = int(train_cfg.get("seed", 1) or 0)
        self.pools = {}
        if self.pool_size > 0:
            if not device_path:
                raise ValueError("opponent_pool_size > 0 needs device_rollout (runner key / --device_rollout): the pool is one actor launch with the weights "
                                 "chosen per 32-env block, which only the device path has")
            from .opponent_pool import OpponentPool, RecurrentOpponentPool
            from .actor_critic import ActorCritic, ActorCriticRecurrent
            module, pool = (ActorCriticRecurrent, RecurrentOpponentPool) if self.recurrent else (ActorCritic, OpponentPool)
            for a in AGENTS:
                view, policy_cfg = self.views[a], self.runners[a].policy_cfg

                def make_actor_critic(view=view, policy_cfg=policy_cfg):      # the private module of one snapshot member: the shapes of the agent's own
                    critic_obs = view.num_privileged_obs if view.num_privileged_obs is not None else view.num_obs      # (push(state_dict) loads the critic too)
                    return module(view.num_obs, critic_obs, view.num_actions, **policy_cfg).to(device)
                self.pools[a] = pool(fused[a], make_actor_critic, self.pool_size, a, seed=self.seed, latest_share=self.latest_share,
                                     num_envs=env.num_envs)
            for a in AGENTS:                              # a view's opponent: the pool of the OTHER agent's versions
                self.views[a].opponent = self.pools["prey" if a == "pred" else "pred"]
            if self.recurrent:                            # raises the LDS limits of the pooled recurrent kernels here, outside any capture
                env.shared_actor_launch(fused["pred"], self.pools["prey"])
        self.current_evolution = 0
        if log_dir is not None:
            for a in AGENTS:
                self._follow(a)

    def _check_policy_class(self, train_cfg, device):
        """Whether the policies are recurrent.  ``ActorCriticRecurrent`` is taken only where the device path can run it; every other case
        raises with its reason before anything is built."""
        name = self.cfg.get("policy_class_name", "ActorCritic")
        pool_recurrent, pool_size = bool(self.cfg.get("opponent_pool_recurrent", False)), int(self.cfg.get("opponent_pool_size", 0) or 0)
        if pool_recurrent and name == "ActorCritic":
            raise ValueError("opponent_pool_recurrent with feed-forward policies: the key makes the pools of two ActorCriticRecurrent policies "
                             "(--policy_class_name ActorCriticRecurrent); a feed-forward pool needs opponent_pool_size alone")
        if pool_recurrent and pool_size <= 0:
            raise ValueError("opponent_pool_recurrent without an opponent pool: set the runner key opponent_pool_size > 0 (--opponent_pool K)")
        if name == "ActorCritic":
            return False
        if name != "ActorCriticRecurrent" or not self.cfg.get("device_rollout", False):
            raise NotImplementedError(f"DecGamePolicyRunner trains two feed-forward ActorCritic policies, or two ActorCriticRecurrent policies with the "
                                      f"runner key device_rollout (--device_rollout); policy class {name!r} is not supported for the decentralised game "
                                      "without it: there is no generic loop for two recurrent agents")
        if not str(device).startswith("cuda"):
            raise ValueError(f"ActorCriticRecurrent on dec_high_level_game needs a GPU: the policies are on {device}, the recurrent game kernels run on "
                             "the device and there is no generic loop for two recurrent agents")
        if pool_size > 0 and not pool_recurrent:
            raise ValueError("opponent_pool_size > 0 with ActorCriticRecurrent: the opponent pool is feed-forward (lg_dec_pool_act has no recurrent role); "
                             "set the runner key opponent_pool_recurrent (--opponent_pool_recurrent) for pools of recurrent snapshots")
        import torch.nn as nn
        from .recurrent_actor import gru_unsupported_reason, lstm_unsupported_reason, wide_memory_would_help
        wide = bool(self.cfg.get("wide_memory", False))
        if wide and pool_recurrent:
            raise ValueError("wide_memory with opponent_pool_recurrent: the pooled launches (lg_dec_pool_lstm_step / lg_dec_pool_lstm_act) stop at "
                             "256 units and read main-library handles; a wide recurrent opponent pool does not exist")
        policy = train_cfg["policy"]
        kind = str(policy.get("rnn_type", "lstm")).lower()
        if kind not in ("lstm", "gru"):
            raise ValueError(f"rnn_type must be 'lstm' or 'gru', got {kind!r}")
        probe = (nn.GRU if kind == "gru" else nn.LSTM)(input_size=3, hidden_size=int(policy.get("rnn_hidden_size", 256)),
                                                       num_layers=int(policy.get("rnn_num_layers", 1)))      # (the predator's memory; both have these units)
        if bool(self.cfg.get("dec_gru_shared", False)) and not (kind == "gru" and bool(self.cfg.get("device_gru", False))):
            raise ValueError("dec_gru_shared without GRU memories on the device: the key puts two GRU policies on lg_dec_gru_step -> lg_dec_game_lstm_act "
                             "and needs rnn_type 'gru' (--rnn_type gru) together with the runner key device_gru (--device_gru)")
        if kind == "gru" and bool(self.cfg.get("device_gru", False)):          # opt-in: GRU memories on liblegged_gru.so (separate launches without dec_gru_shared)
            if pool_recurrent:
                raise ValueError("device_gru with opponent_pool_recurrent: the pooled launches (lg_dec_pool_lstm_step / lg_dec_pool_lstm_act) read "
                                 "lg_lstm handles; a recurrent opponent pool of GRU policies does not exist")
            why = gru_unsupported_reason(probe)
            if why is not None:
                raise ValueError(f"ActorCriticRecurrent on dec_high_level_game with device_gru: no device GRU cell for a {why} (wide_memory does not "
                                 "cover a GRU), and there is no generic loop for two recurrent agents")
            return True
        why = lstm_unsupported_reason(probe, wide)
        if why is not None:
            hint = " (the runner key wide_memory / --wide_memory covers up to 512 units)" if not wide and wide_memory_would_help(probe) else ""
            raise ValueError(f"ActorCriticRecurrent on dec_high_level_game: no device LSTM cell for a {why}, and there is no generic loop for two "
                             f"recurrent agents{hint}")
        return True

    def _follow(self, agent):
        """Keep the combined files current while ``agent`` 's runner trains: whenever it saves ``model_<it>.pt`` (``runner.save_interval`` and the end
        of ``learn``) the combined checkpoint is written as well, and every iteration it logs adds a row to ``<log_dir>/progress.csv``."""
        runner, other = self.runners[agent], self.runners["prey" if agent == "pred" else "pred"]
        save, log = runner.save, runner._log_scalars

        def save_both(path, infos=None):
            save(path, infos)
            m = re.search(r"model_(\d+)\.pt$", path)
            if m:
                it = int(m.group(1))
                self.save(os.path.join(self.log_dir, f"model_{it + other.current_learning_iteration}.pt"), iters={agent: it})

        def log_both(it, *args, **kw):
            row = log(it, *args, **kw)
            self._log_row(it + other.current_learning_iteration, agent, it)
            return row
        runner.save, runner._log_scalars = save_both, log_both

    def _sampling_policy(self, agent):
        ac = self.runners[agent].alg.actor_critic

        def act(obs):
            with torch.no_grad():
                return ac.act(obs)
        return act

    @staticmethod
    def agent_of(evolution):
        """The agent trained in evolution ``evolution``: the predator when even, the prey when odd."""
        return AGENTS[evolution % 2]

    @property
    def current_learning_iteration(self):
        return sum(r.current_learning_iteration for r in self.runners.values())

    def learn(self, max_num_evolutions, num_learning_iterations, init_at_random_ep_len=False):
        if init_at_random_ep_len:                          # once, before the first evolution
            self.env.episode_length_buf[:] = torch.randint_like(self.env.episode_length_buf, high=int(self.env.max_episode_length))
            if hasattr(self.env, "refresh_privileged_observations"):
                self.env.refresh_privileged_observations()        # (the privileged rows hold the episode clock)
        for e in range(self.current_evolution, self.current_evolution + max_num_evolutions):
            agent = self.agent_of(e)
            runner = self.runners[agent]
            counted = None
            if self.pools:
                other = "prey" if agent == "pred" else "pred"
                self.pools[agent].push(runner.alg.actor_critic.state_dict(), pushed_at=e)      # at the START: the pool holds strictly earlier versions than its live member
                generator = torch.Generator().manual_seed((self.seed * 1000003 + e) & 0x7FFFFFFFFFFFFFFF)
                if self.priority > 0:
                    self.pools[other].assign(generator, self.opponent_weights(agent))
                else:
                    self.pools[other].assign(generator)    # before learn captures its graph
                if getattr(self.env, "_outcome", None) is not None:
                    self.env.enable_member_outcomes(self.pools[other])             # before learn captures its graph, too
                    counted = (self.pools[other], self.pools[other].member_totals_host())
            if self.recurrent:
                runner._fused.reset_critic_state()         # the critic memory did not move while this agent was the opponent (G21)
            runner.learn(num_learning_iterations=num_learning_iterations, init_at_random_ep_len=False)
            if runner._fused is not None:
                runner._fused.sync_device()                # the other view's opponent: this agent's new weights (both LSTMs and the actor), repacked in place
            if counted is not None and self.log_dir is not None:
                self._log_opponents(e, agent, *counted)
            self.current_evolution = e + 1
            if self.log_dir is not None:
                self.save(os.path.join(self.log_dir, f"model_{self.current_learning_iteration}.pt"))

    def opponent_weights(self, agent):
        """``pfsp_weights`` of the snapshots 1 .. ``filled`` of the pool that ``agent`` plays against, from that pool's running counts (one
        synchronising copy): ``agent`` 's wins and episodes against every snapshot, to the power ``opponent_priority``."""
        from .opponent_pool import pfsp_weights
        pool = self.pools["prey" if agent == "pred" else "pred"]
        rows = pool.member_totals_host()[1:]
        episodes = [r["episodes"] for r in rows]
        wins = [r["captured"] if agent == "pred" else r["episodes"] - r["captured"] for r in rows]
        return pfsp_weights(wins, episodes, self.priority)

    def _log_opponents(self, evolution, agent, pool, before):
        """``<log_dir>/opponents.csv``: one row per member 0 .. ``filled`` of the pool ``agent`` has just played against -- the evolution that
        pushed it (empty for the live member 0), its 32-env blocks, the six outcome counts of THIS evolution (the running counts now less
        ``before``) and ``agent`` 's win rate in them (empty without an episode)."""
        from .. import capi
        from .opponent_pool import learner_win_rate
        os.makedirs(self.log_dir, exist_ok=True)
        path = os.path.join(self.log_dir, "opponents.csv")
        new = not os.path.isfile(path)
        blocks = torch.bincount(pool._slots_host.clamp(0, pool.capacity).long(), minlength=pool.filled + 1).tolist()
        with open(path, "a") as fh:
            if new:
                fh.write(",".join(OPPONENT_COLUMNS) + "\n")
            for m, (now, then) in enumerate(zip(pool.member_totals_host(), before)):
                row = {k: now[k] - then[k] for k in capi.DEC_OUTCOME_COUNTS}
                pushed = "" if m == 0 or pool.pushed_at[m - 1] is None else pool.pushed_at[m - 1]
                rate = learner_win_rate(row, agent)
                fh.write(",".join(str(v) for v in (evolution, agent, m, pushed, blocks[m], *(row[k] for k in capi.DEC_OUTCOME_COUNTS),
                                                   "" if rate != rate else repr(rate))) + "\n")

    def _log_row(self, iteration, agent, agent_iteration):
        """``<log_dir>/progress.csv``: one row per iteration with an ``agent`` column (the per-agent runners write the full scalar tables under
        ``<log_dir>/pred`` and ``<log_dir>/prey``)."""
        os.makedirs(self.log_dir, exist_ok=True)
        path = os.path.join(self.log_dir, "progress.csv")
        new = not os.path.isfile(path)
        with open(path, "a") as fh:
            if new:
                fh.write("iteration,evolution,agent,agent_iteration\n")
            fh.write(f"{iteration},{self.current_evolution},{agent},{agent_iteration}\n")

    def _half(self, agent, it=None):
        r = self.runners[agent]
        return {"model_state_dict": r.alg.actor_critic.state_dict(), "optimizer_state_dict": r.alg.optimizer.state_dict(),
                "iter": r.current_learning_iteration if it is None else it, "infos": None}

    def save(self, path, iters=None):
        """``iters``: agent -> iteration to record for it (a save in the middle of that agent's ``learn``, whose own count moves at the end)."""
        iters = iters or {}
        os.makedirs(os.path.dirname(path), exist_ok=True)
        halves = {a: self._half(a, iters.get(a)) for a in AGENTS}
        d = {"pred": halves["pred"], "prey": halves["prey"], "evolution": self.current_evolution, "iter": halves["pred"]["iter"] + halves["prey"]["iter"]}
        if self.pools:                                     # the snapshots, so that a resumed run meets the same mixture
            d["pool"] = {a: self.pools[a].state() for a in AGENTS}
        torch.save(d, path)

    def load(self, path, load_optimizer=True):
        d = torch.load(path, map_location=self.device, weights_only=True)
        for a in AGENTS:
            r, half = self.runners[a], d[a]
            check_critic_width(r.alg.actor_critic, half["model_state_dict"], a)
            r.alg.actor_critic.load_state_dict(half["model_state_dict"])
            if load_optimizer:
                r.alg.optimizer.load_state_dict(half["optimizer_state_dict"])
                if hasattr(r.alg, "after_optimizer_load"):
                    r.alg.after_optimizer_load()
            if r._fused is not None:
                r._fused.sync_device()
            r.current_learning_iteration = half["iter"]
        self.current_evolution = d["evolution"]
        if self.pools and "pool" in d:                     # checkpoints without it load as before: the pools start empty
            for a in AGENTS:
                self.pools[a].load_state(d["pool"][a])
        return None

    def get_inference_policy(self, agent, device=None):
        if agent not in AGENTS:
            raise ValueError(f"agent must be one of {AGENTS}, got {agent!r}")
        return self.runners[agent].get_inference_policy(device=device)
