"""``DecHighLevelGame`` -- the decentralised predator-prey task of the reference (``legged_gym/envs/a1_game/dec_high_level_game.py``) on the
device.

One env holds a *prey* (the A1 robot, driven by a frozen low-level locomotion policy) and a *predator* (a kinematic point, a single
integrator).  Unlike ``HighLevelGame`` the two are separate agents: the prey policy maps 16 observations (four past sensed relative predator
positions, four visibility flags) to its command ``(lin_vel_x, lin_vel_y, ang_vel_yaw, heading)``, the predator policy maps 3 observations
(the prey's position relative to it) to its velocity ``(vx, vy)``, and each has its own reward.

``step(command_pred, command_prey)`` (reference :169-258) is four launches with no host in between:

    lg_dec_game_pre  ->  low-level actor (lg_policy_act)  ->  lg_step  ->  lg_dec_game_post

``step_policy(fused_pred, fused_prey)`` runs both agents' actors on the device as well, in three launches:

    lg_dec_game_act (three actors + the clips)  ->  lg_step  ->  lg_dec_game_post

With recurrent policies (two ``rl.RecurrentFusedActor``) it is four, ``lg_dec_lstm_step`` (the actor memories of both agents and the critic
memories the caller asks for, one launch) and ``lg_dec_game_lstm_act`` (include/legged_dec_game_recurrent.h: the three actors on the actor
memories' outputs, with the clips) taking ``lg_dec_game_act``'s place.  Two GRU policies (``RecurrentFusedActor(gru=True)``) take six separate
launches for the policy stage; with ``shared_gru=True`` on both (the runner key ``dec_gru_shared``) the cell launch is ``lg_dec_gru_step``
(include/legged_dec_game_gru.h) and the actor launch the same ``lg_dec_game_lstm_act``, which reads only ``h``.

Outcome statistics (off by default; ``env.outcome_stats = True`` on the config object or ``enable_outcome_stats()``): the last launch of
every step path becomes ``lg_dec_outcome_post`` (include/legged_dec_game_outcome.h), which writes what ``lg_dec_game_post`` writes, bit for
bit, and also counts inside the launch why the done envs' episodes ended.  ``extras["episode"]`` then additionally holds five device scalars
``outcome_*`` -- the shares of captures, game time-outs, falls and low-level time-outs among the done envs and their mean episode length --
and ``outcome_totals()`` the running integer sums.  A step is still three launches and a rollout still one graph replay.

``step_policy`` / ``make_graphed_policy_step`` take an ``rl.OpponentPool`` in place of either ``FusedActor``: the actor launch is then
``lg_dec_pool_act`` (include/legged_dec_game_pool.h), the same launch with that role's weights chosen per 32-env block from the pool.

With recurrent policies the pool is an ``rl.RecurrentOpponentPool`` and the two launches of the policy stage are ``lg_dec_pool_lstm_step`` /
``lg_dec_pool_lstm_act`` (include/legged_dec_pool_recurrent.h): the weights of that role's actor memory and actor MLP chosen per block.

Outcomes per pool member (off by default; ``enable_member_outcomes(pool)``, needs the outcome statistics): the last launch becomes
``lg_dec_member_outcome_post`` (include/legged_dec_game_member_outcome.h), ``lg_dec_outcome_post`` that also keeps the six counts per member
of that pool, read back with ``pool.member_totals_host()``.  Everything else comes out bit-identical.

Privileged observations (off by default; ``cfg.env.num_privileged_obs_prey = 22`` and / or ``num_privileged_obs_predator = 10``): an
asymmetric critic.  The critic exists during training only, so it may read what the prey's sensor hides: ``_post`` then issues one more
launch, ``lg_dec_game_privileged_obs`` (include/legged_dec_game_privileged.h), right behind the post launch on every step path, which writes
the agent's critic row from the post-reset state -- the observations, the true relative position, the prey's yaw-forward vector and the
episode clock; for the predator the prey's velocity and current visibility flag as well.  The buffers alternate
with the observation pair, ``step_policy(privileged_out=...)`` lets the launch write straight into a caller's storage, and with both fields
``None`` no library is loaded and no launch is added.

``agent_view(agent, opponent)`` gives one agent's single-agent surface (what ``rl.OnPolicyRunner`` drives) with the other agent acting
inside every step.  Deliberate differences from the reference are listed in DESIGN.md section 8 ("Quirks", G10 onward)."""
import torch

from legged_games_gym_amd import LEGGED_GYM_ROOT_DIR, capi
from legged_games_gym_amd.utils.helpers import class_to_dict

from .game_base import GameBase

SEED_OFFSET_PREY = 7919                      # noise seeds of the two sampled actors: cfg.seed + these (they share the purposes 100 + g, so they must differ)
SEED_OFFSET_PRED = 7919 + 104729
SUMS = ("evasion", "pursuit", "termination")     # rows of the device episode sums / entries of episode_means (include/legged_dec_game.h)
AGENTS = ("pred", "prey")
PRIVILEGED_WIDTHS = {"pred": capi.LG_DEC_NUM_PRIV_PRED, "prey": capi.LG_DEC_NUM_PRIV_PREY}     # include/legged_dec_game_privileged.h


def check_privileged_widths(num_privileged_obs_prey, num_privileged_obs_predator):
    """The two config fields ``env.num_privileged_obs_prey`` / ``env.num_privileged_obs_predator``: each ``None`` (that agent's critic reads its
    observations) or the one width ``lg_dec_game_privileged_obs`` is compiled for.  Returns the agents that are on."""
    want = (capi.LG_DEC_NUM_PRIV_PREY, capi.LG_DEC_NUM_PRIV_PRED)
    got = (num_privileged_obs_prey, num_privileged_obs_predator)
    if any(g is not None and (isinstance(g, bool) or g != w) for g, w in zip(got, want)):
        raise ValueError(f"dec_high_level_game is compiled for {want[0]} prey and {want[1]} predator privileged observations (or None for either), "
                         f"got {got}")
    return tuple(a for a, g in (("pred", num_privileged_obs_predator), ("prey", num_privileged_obs_prey)) if g is not None)


class DecHighLevelGame(GameBase):
    TASK = "dec_high_level_game"
    GRAPHED_ACTORS = "FusedActors"
    OUTCOME_COUNTS, OUTCOME_MEANS, OUTCOME_BUFFERS = capi.DEC_OUTCOME_COUNTS, capi.DEC_OUTCOME_MEANS, staticmethod(capi.dec_outcome_buffers)
    OUTCOME_TICKET = OUTCOME_ONLY_EPISODE = False     # (the reduction shares the game's extras_ticket; extras["episode"] also holds the reward means)

    def __init__(self, cfg, sim_params, physics_engine, sim_device, headless):
        self._init_low_level(cfg, sim_params, physics_engine, sim_device, headless, LEGGED_GYM_ROOT_DIR)
        self._parse_cfg(self.cfg)
        self.num_envs = cfg.env.num_envs
        self.num_obs_prey = cfg.env.num_observations_prey
        self.num_privileged_obs_prey = cfg.env.num_privileged_obs_prey
        self.num_actions_prey = cfg.env.num_actions_prey
        self.num_obs_pred = cfg.env.num_observations_predator
        self.num_privileged_obs_pred = cfg.env.num_privileged_obs_predator
        self.num_actions_pred = cfg.env.num_actions_predator
        sizes = (self.num_obs_prey, self.num_actions_prey, self.num_obs_pred, self.num_actions_pred)
        if sizes != (capi.LG_DEC_NUM_OBS_PREY, capi.LG_DEC_NUM_ACTIONS_PREY, capi.LG_DEC_NUM_OBS_PRED, capi.LG_DEC_NUM_ACTIONS_PRED):
            raise ValueError(f"dec_high_level_game is compiled for 16 / 4 prey and 3 / 2 predator observations / actions, got {sizes}")
        self._privileged = check_privileged_widths(self.num_privileged_obs_prey, self.num_privileged_obs_pred)
        if self._privileged:
            capi.load_dec_game_privileged_library()            # raises when it is not built: no launch is quietly left out
        if self.ll_env.num_dof != capi.LG_MAX_DOF:
            raise ValueError("dec_high_level_game resets the 12 joints of the low-level robot")
        self.privileged_obs_buf_prey = self.privileged_obs_buf_pred = None
        self._priv_pair = {a: None for a in AGENTS}
        self.extras = {}
        self.enable_viewer_sync = True
        self.viewer = None
        self._init_buffers()
        self._prepare_reward_functions()
        self._pack()
        self._outcome = None
        self._member_pool = self._member_outcome = None
        if getattr(cfg.env, "outcome_stats", False):           # no field of the registered config classes: they stay value for value the reference's
            self.enable_outcome_stats()
        if self._privileged:
            self._write_privileged()                           # valid from construction on
        self.init_done = True

    # ------------------------------------------------------------------ hot path
    def _flip_observations(self, carry):
        """The caller may still hold the observations returned last time (PPO.act keeps them until process_env_step, and the reference builds
        new tensors every step, :377, :391): alternate between two buffers per agent, carrying the prey's history over when ``carry``."""
        prev = self.obs_buf_prey
        self._obs_flip ^= 1
        self._select_observations()
        if carry:
            self.obs_buf_prey.copy_(prev)
        return prev

    def _unflip_observations(self):
        self._obs_flip ^= 1
        self._select_observations()

    def _select_observations(self):
        """Both agents' buffers and the privileged ones on the current side of their pairs."""
        self.obs_buf_prey = self._obs_pair_prey[self._obs_flip]
        self.obs_buf_pred = self._obs_pair_pred[self._obs_flip]
        self._select_privileged()

    def _select_privileged(self):
        """The privileged buffers alternate with the observations, for the same reason: ``PPO.act`` keeps the critic observations until
        ``process_env_step``."""
        for a in self._privileged:
            setattr(self, f"privileged_obs_buf_{a}", self._priv_pair[a][self._obs_flip])

    def refresh_privileged_observations(self):
        """Write the privileged rows again from the current state, after the caller edited what they are taken from (a runner that
        randomises ``episode_length_buf`` at start).  Nothing to do with both config fields ``None``."""
        if self._privileged:
            self._write_privileged()

    def _own_privileged(self):
        """Before a capture: the privileged rows back in the env's own pair when the last ``step_policy`` left them in a caller's tensor."""
        for a in self._privileged:
            last = getattr(self, f"privileged_obs_buf_{a}")
            if last is not self._priv_pair[a][self._obs_flip]:
                self._priv_pair[a][self._obs_flip].copy_(last)
        self._select_privileged()

    def _write_privileged(self, B=None, stream=None, out=None):
        """``lg_dec_game_privileged_obs`` on the current state: the rows of the agents that are on, into the env's current buffers or into
        the caller's tensors ``out`` (agent -> tensor), which the env then hands out as that agent's privileged observations."""
        if B is None:                                          # from the host (construction, reset_idx): into the env's own pair
            self._select_privileged()
            B = capi.dec_game_buffers(dict(self._pointers, obs_pred=self.obs_buf_pred.data_ptr(), obs_prey=self.obs_buf_prey.data_ptr()))
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        for a, t in (out or {}).items():
            setattr(self, f"privileged_obs_buf_{a}", t)
        dst = {a: getattr(self, f"privileged_obs_buf_{a}") for a in AGENTS}
        capi.dec_game_privileged_obs(self._P, B, *(None if dst[a] is None else dst[a].data_ptr() for a in AGENTS), stream)

    def step(self, command_pred, command_prey):
        """Apply both agents' commands, run one low-level policy step, advance the predator (reference :169-210).  ``command_pred`` [num_envs, 2]
        and ``command_prey`` [num_envs, 4] are clipped IN PLACE, as in the reference."""
        ll = self.ll_env
        self._flip_observations(carry=True)
        B = self._bind(command_pred, command_prey, self.obs_buf_pred, self.obs_buf_prey)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        capi.dec_game_pre(self._P, B, stream)
        actions = self.ll_policy(ll.obs_buf)
        ll.step(actions)
        self._post(B, ll.common_step_counter, stream)
        return self._step_result()

    def _post(self, B, common_step_counter, stream, privileged_out=None):
        """The post stage of every step path: ``lg_dec_game_post``, or ``lg_dec_outcome_post`` with the outcome statistics on, or
        ``lg_dec_member_outcome_post`` with them on and a pool bound (``enable_member_outcomes``); with privileged observations on,
        ``lg_dec_game_privileged_obs`` right behind whichever ran."""
        if self._outcome is None:
            capi.dec_game_post(self._P, B, common_step_counter, stream)
        elif self._member_outcome is None:
            capi.dec_outcome_post(self._P, B, self._outcome, common_step_counter, stream)
        else:
            capi.dec_member_outcome_post(self._P, B, self._outcome, self._member_outcome, common_step_counter, stream)
        if self._privileged:
            self._write_privileged(B, stream, privileged_out)

    # ------------------------------------------------------------------ outcome statistics
    def enable_member_outcomes(self, pool):
        """Keep the outcome counts per member of ``pool`` (an ``rl.OpponentPool``) as well, or stop doing so (``None``).  With a pool bound and
        the outcome statistics on, ``_post`` issues ``lg_dec_member_outcome_post`` on every step path, given the pool's slot table, ``count = 1 +
        capacity`` and the pool's count buffers: an episode is counted for the member its 32-env block has in the step in which it ends
        (DESIGN.md section 8, G20).  Everything ``lg_dec_outcome_post`` writes is unchanged; read the counts with
        ``pool.member_totals_host()``.  A graph captured earlier keeps the launch it was captured with."""
        if pool is None:
            self._member_pool = self._member_outcome = None
            return
        if self._outcome is None:
            raise RuntimeError("outcomes per pool member need the outcome statistics: call enable_outcome_stats() (or set env.outcome_stats = True) first")
        self._member_pool = pool                                   # keeps the buffers alive
        self._member_outcome = capi.dec_member_outcome_buffers({"block_slot": pool.slot_table(self.num_envs).data_ptr(), "member_accum": pool.member_accum.data_ptr(),
                                                                "member_totals": pool.member_totals.data_ptr()}, 1 + pool.capacity)

    def _step_result(self):
        return (self.obs_buf_pred, self.obs_buf_prey, self.privileged_obs_buf_pred, self.privileged_obs_buf_prey, self.rew_buf_pred, self.rew_buf_prey,
                self.reset_buf, self.extras)

    def _device_step(self, command_pred, command_prey):
        """``step`` for graph capture: the step counter is the low-level env's device counter, observations stay in one buffer per agent."""
        ll = self.ll_env
        B = self._bind(command_pred, command_prey, self.obs_buf_pred, self.obs_buf_prey)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        capi.dec_game_pre(self._P, B, stream)
        actions = self.ll_policy(ll.obs_buf)
        ll._sim.step(actions, -1)
        self._post(B, -1, stream)

    def make_graphed_step(self, policy_pred, policy_prey, warmup=3, steps_per_replay=1):
        """Capture ``step(policy_pred(obs_buf_pred), policy_prey(obs_buf_prey))`` into one HIP graph and return a zero-argument callable that
        replays it: both policies, ``lg_dec_game_pre``, low-level actor, ``lg_step``, ``lg_dec_game_post`` -- no host in between.  The
        policies must be capturable and read ``self.obs_buf_pred`` / ``self.obs_buf_prey``."""
        self._own_privileged()
        self._step_graph, replay = self._capture(lambda: self._device_step(policy_pred(self.obs_buf_pred), policy_prey(self.obs_buf_prey)), warmup, steps_per_replay, self._step_result)
        return replay

    # ------------------------------------------------------------------ hot path with both actors on the device
    def _who_acts(self, fused_pred, fused_prey):
        """The pair of a policy step, resolved once: ``(live, pools, recurrent)``, the first two by agent.  ``fused_*`` may each be an
        ``rl.OpponentPool`` (``rl.RecurrentOpponentPool``) instead of an actor: ``pools`` then holds it (else None) and ``live`` its live actor,
        which supplies seed, step source, output buffers and, recurrent, the state.  ``recurrent``: ``_recurrent_pair``, with its refusals."""
        pools = {a: f if getattr(f, "is_opponent_pool", False) else None for a, f in zip(AGENTS, (fused_pred, fused_prey))}
        live = {"pred": _live(fused_pred), "prey": _live(fused_prey)}
        return live, pools, self._recurrent_pair(live["pred"], live["prey"], pools["pred"], pools["prey"])

    @staticmethod
    def _slot_args(pools, n):
        """What a pooled launch takes per agent, predator first: ``pool handle, address of its slot table`` (read per call), or ``None, None``."""
        return [a for pool in (pools["pred"], pools["prey"]) for a in ((pool.handle, pool.slot_table(n).data_ptr()) if pool is not None else (None, None))]

    def _cell_launch(self, roles, gru, slots, stream):
        """The shared cell launch on four role entries (``RecurrentFusedActor.cell_roles`` of the predator, then of the prey):
        ``lg_dec_gru_step`` for a GRU pair (the entries hold one state tensor each way), ``lg_dec_pool_lstm_step`` given ``slots``
        (``_slot_args``: the weights of a pooled actor memory per 32-env block), else ``lg_dec_lstm_step``.  Rows that ``reset_buf`` of the
        previous step marks start from a zero state."""
        if gru:
            capi.dec_gru_step(roles, self.reset_buf.data_ptr(), self.num_envs, stream)
        elif slots is not None:
            capi.dec_pool_lstm_step(roles, *slots, self.reset_buf.data_ptr(), self.num_envs, stream)
        else:
            capi.dec_lstm_step(roles, self.reset_buf.data_ptr(), self.num_envs, stream)

    def _actor_launch(self, live, slots, B, ll_actions, mean, h, obs, det, outputs, stream):
        """The shared actor launch, the three actors and both clips: ``lg_dec_game_act`` on the observations, with ``h`` (the two actor
        memories' outputs) ``lg_dec_game_lstm_act`` on those; given ``slots`` (``_slot_args``) the pooled ``lg_dec_pool_act`` /
        ``lg_dec_pool_lstm_act``, which take a pooled role's weights, biases and std per 32-env block from the member its slot table names.
        ``live``, ``mean``, ``h``, ``obs``, ``det`` (deterministic), ``outputs`` are by agent; an observation tensor may be None in the recurrent
        warm-up, ``outputs`` are ``capi.lg_dec_act_outputs`` or None.  Returns rc: 0, or -4 when the actor triple or the wide precision has
        no shared kernel and nothing was launched; no noise stream is advanced here."""
        ptr = lambda t: None if t is None else t.data_ptr()
        pred, prey = live["pred"], live["prey"]
        step, ctr = prey.peek_step()
        front = (pred.handle, prey.handle, self._ll_fused.handle, *(slots or ()), self._P, B)
        tail = (ptr(obs["pred"]), ptr(obs["prey"]), self.ll_env.obs_buf.data_ptr(), ll_actions.data_ptr(), mean["pred"].data_ptr(), mean["prey"].data_ptr(),
                pred.seed, prey.seed, step, ctr, det["pred"], det["prey"], outputs["pred"], outputs["prey"], stream)
        if h is None:
            return (capi.dec_game_act if slots is None else capi.dec_pool_act)(*front, *tail)
        return (capi.dec_game_lstm_act if slots is None else capi.dec_pool_lstm_act)(*front, h["pred"].data_ptr(), h["prey"].data_ptr(), *tail)

    def _act(self, fused_pred, fused_prey, obs_pred_in, obs_prey_in, obs_pred_out, obs_prey_out, deterministic_pred, deterministic_prey, out_pred=None, out_prey=None,
             with_critic_memory=(), critic_obs=None):
        """``lg_dec_game_act``: both commands = clip(actor(obs) + noise), the prey's into the low-level commands, the low-level actions, and
        the prey's observations copied to ``obs_prey_out`` (where ``lg_dec_game_post`` then shifts the history in place) -- one launch.
        Separate launches when the actor triple or the wide precision has no shared kernel (rc -4, decided per call:
        ``lg_mlp_wide_set_precision`` may change between calls): ``lg_policy_act`` x 3 + ``lg_dec_game_pre``.  ``out_*``: dicts of optional
        float32 outputs ``sample`` / ``sigma`` / ``log_prob`` / ``obs_copy`` (the rollout storage's copy of the observations read).
        ``fused_pred`` / ``fused_prey`` may each be an ``rl.OpponentPool`` instead of a ``FusedActor`` (``_who_acts``): the launch is then
        ``lg_dec_pool_act`` (include/legged_dec_game_pool.h).  Its rc -4 path is one ``lg_policy_act`` on all envs per member in use, rows
        selected by block.
        Two ``RecurrentFusedActor`` s: the memory stage first (``_step_memories``; ``with_critic_memory``: the agents whose critic memory
        moves too; ``critic_obs``: agent -> what that memory reads, None = the agent's observations), then ``lg_dec_game_lstm_act`` on the
        two new ``h`` -- ``lg_dec_pool_lstm_act`` given an ``rl.RecurrentOpponentPool`` (include/legged_dec_pool_recurrent.h).  Separate
        launches (``lg_lstm_actor_act`` x 2, per member in use and rows selected by block for a pooled role, + ``lg_dec_game_pre`` +
        low-level ``lg_policy_act``) on rc -4, at wide precision 0 or without the library.
        ``self.last_act_rc``: 0 when the shared actor launch ran, else -4.
        Returns ``(command_pred, mean_pred), (command_prey, mean_prey), ll_actions, buffers``."""
        ll, n = self.ll_env, self.num_envs
        live, pools, recurrent = self._who_acts(fused_pred, fused_prey)
        obs, det = {"pred": obs_pred_in, "prey": obs_prey_in}, {"pred": deterministic_pred, "prey": deterministic_prey}
        for name, t, width in (("predator", obs_pred_in, self.num_obs_pred), ("prey", obs_prey_in, self.num_obs_prey)):
            if t.shape != (n, width) or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"{name} observations must be a contiguous float32 [{n},{width}] tensor")
        out = {"pred": dict(out_pred or {}), "prey": dict(out_prey or {})}
        for o, na, no in ((out["pred"], self.num_actions_pred, self.num_obs_pred), (out["prey"], self.num_actions_prey, self.num_obs_prey)):
            unknown = set(o) - {"sample", "sigma", "log_prob", "obs_copy"}
            if unknown:
                raise ValueError(f"unknown optional outputs {sorted(unknown)}")
            self._check_output("sample", o.get("sample"), n * na)
            self._check_output("sigma", o.get("sigma"), n * na)
            self._check_output("log_prob", o.get("log_prob"), n)
            self._check_output("obs_copy", o.get("obs_copy"), n * no)
        command, mean = {}, {}
        for a in AGENTS:
            command[a], mean[a] = live[a].output_buffers(n)
        result = (command["pred"], mean["pred"]), (command["prey"], mean["prey"])
        ll_actions = self._ll_fused.output_buffers(n)[0]
        B = self._bind(command["pred"], command["prey"], obs_pred_out, obs_prey_out)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        ptr = lambda t: None if t is None else t.data_ptr()
        carry = obs_prey_out is not obs_prey_in

        def outputs(o, extra_copy):
            s = capi.lg_dec_act_outputs()
            s.sample, s.sigma, s.log_prob = ptr(o.get("sample")), ptr(o.get("sigma")), ptr(o.get("log_prob"))
            s.obs_copy = ptr(o.get("obs_copy")) if o.get("obs_copy") is not None else extra_copy
            return s
        # the kernel has one observation copy per agent: the prey's goes to the other ping-pong buffer (history carry) unless the caller asks
        # for its own copy, in which case the carry is a separate copy below
        want_prey_copy = out["prey"].get("obs_copy") is not None
        if live["prey"].peek_step() != live["pred"].peek_step():
            raise ValueError("the two FusedActors must count their noise steps alike (both on the low-level sim's device step counter, or both on the host)")
        if live["pred"].seed == live["prey"].seed:
            raise ValueError("the two FusedActors need different seeds: they draw their noise under the same purposes")
        pooled = pools["pred"] is not None or pools["prey"] is not None
        slots = self._slot_args(pools, n) if pooled else None
        h, shared, gru = None, True, False
        if recurrent:
            h, shared, gru = self._step_memories(live, pools, slots, obs, with_critic_memory, critic_obs, stream)
        rc = -4                                                # 0: the shared launch ran; -4: the separate launches below
        if shared:
            # a GRU pair on the shared launches stores the log-prob the separate launches store (torch's, below): the launch leaves the
            # unclipped sample for it, in the caller's tensor or in a buffer kept here, and writes no log-prob of its own
            launched = {a: self._gru_log_prob_outputs(a, out[a], live[a]) if gru else out[a] for a in AGENTS}
            structs = {"pred": outputs(launched["pred"], None), "prey": outputs(launched["prey"], obs_prey_out.data_ptr() if carry else None)}
            rc = self._actor_launch(live, slots, B, ll_actions, mean, h, obs, det, structs, stream)
            if rc != 0 and recurrent:
                self._say_separate("no kernel for this actor pair", pooled=pooled)
        self.last_act_rc = rc
        if rc == 0:
            live["pred"].next_step(); live["prey"].next_step()     # the launch used this step of both noise streams
            if carry and want_prey_copy:
                obs_prey_out.copy_(obs_prey_in)
            if gru:
                for a in AGENTS:
                    if out[a].get("log_prob") is not None:       # _fill_optional_outputs' expression on the same sample, mean and std: the same bits
                        out[a]["log_prob"].view(n).copy_(torch.distributions.Normal(mean[a], live[a].ac.std.detach()).log_prob(launched[a]["sample"].view(n, -1)).sum(-1))
            return *result, ll_actions, B
        # nothing was launched: each agent's actor on what it reads (the observations; behind a memory, its output) -- of a pool per member in
        # use, rows by block, std [n, actions] of the rows' members -- then the clips and the low-level actor
        for a in AGENTS:
            x = h[a] if recurrent else obs[a]
            if pools[a] is None:
                (sample, mu), std = (live[a].fused if recurrent else live[a]).act_with_mean(x, det[a]), live[a].ac.std.detach()
            else:
                sample, mu, std = pools[a].act_separate(x, det[a])
            self._fill_optional_outputs(out[a], n, sample, mu, std, obs[a])
        if carry:
            obs_prey_out.copy_(obs_prey_in)
        capi.dec_game_pre(self._P, B, stream)
        ll_actions = self.ll_policy(ll.obs_buf)
        return *result, ll_actions, B

    # ------------------------------------------------------------------ recurrent policies
    @staticmethod
    def _recurrent_pair(fused_pred, fused_prey, pool_pred=None, pool_prey=None):
        """Whether both actors are ``RecurrentFusedActor`` s.  Both agents are recurrent or neither (one train cfg builds both), and next to a
        recurrent actor a pool must be recurrent too (``rl.RecurrentOpponentPool``): an ``OpponentPool`` holds feed-forward snapshots only."""
        rec = [bool(getattr(f, "recurrent", False)) for f in (fused_pred, fused_prey)]
        if any(rec) and any(pool is not None and not getattr(pool, "recurrent", False) for pool in (pool_pred, pool_prey)):
            raise ValueError("the opponent pool is feed-forward: lg_dec_pool_act has no recurrent role, so an OpponentPool cannot stand next to a "
                             "RecurrentFusedActor")
        if rec[0] != rec[1]:
            raise ValueError("both agents of dec_high_level_game are recurrent (RecurrentFusedActor) or neither: lg_dec_game_lstm_act has no mixed pair")
        return rec[0]

    def _recurrent_library(self, fused, say=True, pooled=False):
        """``(library or None, whether lg_dec_game_lstm_act can be used now)``: the low-level role is the split-bf16 kernel, so wide precision
        0 takes the separate actor launches, and a build without the library takes separate launches throughout (a one-line message the
        first time for each reason).  Decided per call: ``lg_mlp_wide_set_precision`` may change between calls.  ``pooled``: the library of
        the pooled launches (``lg_dec_pool_lstm_step`` / ``lg_dec_pool_lstm_act``) instead."""
        lib = self._load_or_say(capi.load_dec_pool_recurrent_library if pooled else capi.load_dec_game_recurrent_library, say, pooled)
        if lib is not None and self._wide_precision_0(fused):
            self._say_separate("wide precision 0", say, pooled)
            return lib, False
        return lib, lib is not None

    def _recurrent_launches(self, fused_pred, fused_prey, say=True, pooled=False):
        """``_recurrent_library`` for a pair of actors.  An actor with ``wide`` memories (``RecurrentFusedActor(wide=True)`` above 256 units) holds
        handles of liblegged_lstm_wide.so, which none of the shared launches reads: separate launches throughout, said once.  Likewise an
        actor with ``gru`` memories (``RecurrentFusedActor(gru=True)``, handles of liblegged_gru.so): ``lg_dec_lstm_step`` reads ``lg_lstm`` handles.
        Two ``gru`` actors that are both ``shared_gru`` (the runner key ``dec_gru_shared``) take ``_gru_shared_launches`` instead."""
        if getattr(fused_pred, "wide", False) or getattr(fused_prey, "wide", False):
            self._say_separate("wide memory", say, pooled)
            return None, False
        if self._gru_shared_pair(fused_pred, fused_prey) and not pooled:
            return self._gru_shared_launches(fused_pred, say=say)
        if getattr(fused_pred, "gru", False) or getattr(fused_prey, "gru", False):
            self._say_separate("GRU memory", say, pooled)
            return None, False
        return self._recurrent_library(fused_pred, say=say, pooled=pooled)

    @staticmethod
    def _gru_shared_pair(fused_pred, fused_prey):
        """Whether both actors hold GRU memories and both ask for the shared launches (``RecurrentFusedActor(gru=True, shared_gru=True)``)."""
        return all(getattr(f, "gru", False) and getattr(f, "shared_gru", False) for f in (fused_pred, fused_prey))

    def _gru_log_prob_outputs(self, agent, out, fused):
        """The optional outputs handed to ``lg_dec_game_lstm_act`` for a GRU pair on the shared launches: ``out`` itself when no log-prob is
        asked for; otherwise ``out`` without its log-prob and with a sample tensor (the caller's, or one kept per agent so that a captured
        graph finds it at the same address), from which ``_act`` then fills the log-prob the way the separate launches do.  The
        key ``dec_gru_shared`` so changes which launches run and not one bit of what a rollout stores."""
        if out.get("log_prob") is None:
            return out
        sample = out.get("sample")
        if sample is None:
            kept = self.__dict__.setdefault("_gru_samples", {})
            if agent not in kept or kept[agent].shape != (self.num_envs, fused.num_actions):
                kept[agent] = torch.empty(self.num_envs, fused.num_actions, device=self.device)
            sample = kept[agent]
        return dict(out, sample=sample, log_prob=None)

    def _gru_shared_launches(self, fused, say=True):
        """``_recurrent_library`` for a GRU pair on the shared launches: ``(liblegged_dec_game_gru.so or None, whether lg_dec_game_lstm_act can
        be used now)``.  The cell launch ``lg_dec_gru_step`` needs only the first; the actor MLP behind a GRU memory is an ``lg_lstm_actor`` on
        ``h``, so the actor launch is the LSTM pair's, under its conditions.  Without the GRU library everything takes the separate launches
        (a one-line message that names it); without liblegged_dec_game_recurrent.so or at wide precision 0 only the actors do."""
        lib = self._load_or_say(capi.load_dec_game_gru_library, say)
        return lib, lib is not None and self._recurrent_library(fused, say=say)[1]

    def _say_separate(self, why, say=True, pooled=False):
        if pooled:
            line = f"[{self.TASK}] pooled recurrent actor launch unavailable ({why}); lg_lstm_actor_act per member + lg_dec_game_pre + lg_policy_act"
        else:
            line = f"[{self.TASK}] recurrent actor launch unavailable ({why}); lg_lstm_actor_act x 2 + lg_dec_game_pre + lg_policy_act"
        self._say_once((why, pooled), say, line)

    def _step_memories(self, live, pools, slots, obs, with_critic_memory, critic_obs, stream):
        """The memory stage of ``_act`` for two ``RecurrentFusedActor`` s (arguments already checked there): both actor memories on the
        observations they read, and the critic memory of every agent in ``with_critic_memory``, in one launch (``_cell_launch``) on the
        actors' own slots (``RecurrentFusedActor.cell_roles``).  ``critic_obs``: agent -> the input of its critic memory (the privileged
        observations that belong to the observations read), None or absent = the observations themselves.  The critic memories' outputs are
        left in ``self._critic_out`` (agent -> tensor, None when it did not move).  Given pools (``slots``) the state is the live actor's
        and the critic memory is never pooled.  Without a library of the shared launches (``_recurrent_launches``) ``lg_lstm_step`` per agent
        instead (a GRU's ``lg_gru_step``), of a pooled role one per member in use on all envs, rows selected by block
        (``step_memory_separate``).  Returns ``(h by agent, whether the shared actor launch can follow, whether the pair is a GRU pair on the
        shared launches)``."""
        n = self.num_envs
        cobs = {a: None if a not in with_critic_memory else obs[a] if (critic_obs or {}).get(a) is None else critic_obs[a] for a in AGENTS}
        lib, shared = self._recurrent_launches(live["pred"], live["prey"], pooled=slots is not None)
        gru = lib is not None and self._gru_shared_pair(live["pred"], live["prey"])
        roles, h, self._critic_out = [], {}, {}
        for a in AGENTS:
            if lib is not None:
                entries, h[a], self._critic_out[a] = live[a].cell_roles(n, obs[a], cobs[a], a)
                roles += entries
            elif pools[a] is None:
                h[a], self._critic_out[a] = live[a].step_memories(obs[a], cobs[a], reset=self.reset_buf)
            else:
                h[a] = pools[a].step_memory_separate(obs[a], reset=self.reset_buf)
                self._critic_out[a] = None if cobs[a] is None else live[a].step_critic_memory(cobs[a], reset=self.reset_buf)
                live[a].advance_slots(cobs[a] is not None)
        if lib is not None:
            self._cell_launch(roles, gru, slots, stream)
            for a in AGENTS:
                live[a].advance_slots(cobs[a] is not None)
        return h, shared, gru

    def shared_actor_launch(self, fused_pred, fused_prey):
        """Whether the actor launch of a step has a kernel for this pair next to the low-level actor at the current wide precision (rc 0, not
        -4).  Issues it once, deterministically, on the current observations when it has: commands, means, low-level commands and actions
        are overwritten (every step path rewrites them before reading them), no noise stream is advanced and no memory moves.  A
        feed-forward pair: ``lg_dec_game_act`` on the live actors, also when a pool is given.  With two ``RecurrentFusedActor`` s the
        warm-up call that raises the LDS limits of both kernels of liblegged_dec_game_recurrent.so outside any capture: one cell launch
        (``_cell_launch``: ``lg_dec_lstm_step``; ``lg_dec_gru_step`` warms up k_dec_gru_cell the same way) of the two actor memories into the
        slots the next step overwrites, then ``lg_dec_game_lstm_act`` on the actor memories' current outputs.  Given an
        ``rl.RecurrentOpponentPool`` for an agent, the pooled kernels of liblegged_dec_pool_recurrent.so are warmed up the same way
        (``lg_dec_pool_lstm_step``, ``lg_dec_pool_lstm_act``)."""
        n = self.num_envs
        live, pools, recurrent = self._who_acts(fused_pred, fused_prey)
        command, mean = {}, {}
        for a in AGENTS:
            command[a], mean[a] = live[a].output_buffers(n)
        ll_actions = self._ll_fused.output_buffers(n)[0]
        B = self._bind(command["pred"], command["prey"], self.obs_buf_pred, self.obs_buf_prey)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        obs, slots, h, shared = {"pred": self.obs_buf_pred, "prey": self.obs_buf_prey}, None, None, True
        if recurrent:
            pooled = pools["pred"] is not None or pools["prey"] is not None
            lib, shared = self._recurrent_launches(live["pred"], live["prey"], say=False, pooled=pooled)
            if lib is None:
                return False
            roles = [entry for a in AGENTS for entry in live[a].cell_roles(n, obs[a], agent=a)[0]]
            h, obs = {a: live[a].hidden_states()[0][0][0] for a in AGENTS}, dict.fromkeys(AGENTS)
            slots = self._slot_args(pools, n) if pooled else None
            self._cell_launch(roles, self._gru_shared_pair(live["pred"], live["prey"]), slots, stream)
        return shared and self._actor_launch(live, slots, B, ll_actions, mean, h, obs, dict.fromkeys(AGENTS, True), dict.fromkeys(AGENTS), stream) == 0

    def step_policy(self, fused_pred, fused_prey, deterministic_pred=False, deterministic_prey=False, out_pred=None, out_prey=None, with_critic_memory=(),
                    privileged_out=None):
        """Rollout step with both agents' actors on the device: ``lg_dec_game_act`` -> ``lg_step`` -> ``lg_dec_game_post``, three launches.
        Returns ``(command_pred, mean_pred), (command_prey, mean_prey), step result``: the clipped commands (what ``step`` leaves in the
        caller's tensors) and the actors' outputs, all in the ``FusedActor`` buffers.  ``out_pred`` / ``out_prey``: dicts of optional float32
        outputs -- ``sample`` (the unclipped sample), ``sigma``, ``log_prob`` of that sample (what ``PPO.act`` stores), ``obs_copy`` (the
        observations the actor read).  The observations the actors read stay in the tensors returned by the previous call, as with ``step``.

        Two ``RecurrentFusedActor`` s make it four launches, ``lg_dec_lstm_step`` -> ``lg_dec_game_lstm_act`` -> ``lg_step`` -> ``lg_dec_game_post``:
        both actor memories advance on their observations, rows whose episode ended in the previous step from a zero state.
        ``with_critic_memory``: the agents ("pred", "prey") whose critic memory advances in the same launch; such an agent's tuple gets the
        critic memory's output of the step as a third value (the actor's buffer, re-used two steps later).  A critic memory that is not
        named stays where it is; a critic memory that moves reads the agent's privileged observations where those are on.

        ``privileged_out``: an optional dict ``{"pred": tensor, "prey": tensor}`` (either key may be absent) of contiguous float32
        ``[num_envs, 10]`` / ``[num_envs, 22]`` destinations for THIS step's new privileged rows: ``lg_dec_game_privileged_obs`` writes there
        instead of into the env's pair, and the step result's privileged slots are those tensors (a runner's rollout storage)."""
        ll = self.ll_env
        privileged_out = self._check_privileged_out(privileged_out)
        with_critic_memory = (with_critic_memory,) if isinstance(with_critic_memory, str) else tuple(with_critic_memory or ())
        unknown = set(with_critic_memory) - set(AGENTS)
        if unknown:
            raise ValueError(f"with_critic_memory names agents of {AGENTS}, got {sorted(unknown)}")
        prev_pred = self.obs_buf_pred
        prev_priv = {a: getattr(self, f"privileged_obs_buf_{a}") for a in AGENTS}
        prev_prey = self._flip_observations(carry=False)
        try:
            pred, prey, ll_actions, B = self._act(fused_pred, fused_prey, prev_pred, prev_prey, self.obs_buf_pred, self.obs_buf_prey, deterministic_pred,
                                                  deterministic_prey, out_pred, out_prey, with_critic_memory, critic_obs=prev_priv)
        except Exception:
            self._unflip_observations()
            for a in self._privileged:
                setattr(self, f"privileged_obs_buf_{a}", prev_priv[a])
            raise
        ll.step(ll_actions)
        self._post(B, -1 if ll._capturing else ll.common_step_counter, torch.cuda.current_stream(self.device).cuda_stream, privileged_out)
        if with_critic_memory and getattr(_live(fused_pred), "recurrent", False):
            pred = pred + (self._critic_out["pred"],) if "pred" in with_critic_memory else pred
            prey = prey + (self._critic_out["prey"],) if "prey" in with_critic_memory else prey
        return pred, prey, self._step_result()

    def _check_privileged_out(self, privileged_out):
        privileged_out = dict(privileged_out or {})
        for a, t in privileged_out.items():
            if a not in AGENTS:
                raise ValueError(f"privileged_out names agents of {AGENTS}, got {a!r}")
            if a not in self._privileged:
                raise ValueError(f"privileged_out[{a!r}]: the privileged observations of this agent are off (cfg.env.num_privileged_obs_*)")
            n, w = self.num_envs, PRIVILEGED_WIDTHS[a]
            if t.shape != (n, w) or t.dtype != torch.float32 or not t.is_contiguous() or str(t.device) != str(self.device):
                raise ValueError(f"privileged_out[{a!r}] must be a contiguous float32 [{n},{w}] tensor on {self.device}")
        return privileged_out

    def make_graphed_policy_step(self, fused_pred, fused_prey, warmup=3, steps_per_replay=1, deterministic_pred=False, deterministic_prey=False,
                                 with_critic_memory=()):
        """``make_graphed_step`` with both actors on the device: the graph is ``lg_dec_game_act`` -> ``lg_step`` -> ``lg_dec_game_post`` per
        step, the observations stay in one buffer per agent.  Both ``FusedActor`` s must draw their noise stream from the low-level sim's
        device step counter (``FusedActor(..., step_counter=env.ll_env._sim.buf["step_counter"])``).  Returns a zero-argument callable that
        replays the graph; the actors' ``output_buffers(num_envs)`` then hold the commands and the means of the last step.
        ``deterministic_pred`` / ``deterministic_prey``: that agent's command is its clipped mean (evaluation).
        Two ``RecurrentFusedActor`` s: only the actor memories are in the cell launch, and the critic memories of the agents named in
        ``with_critic_memory``; with an odd number of steps per replay the slots of BOTH actors are held (``hold_slot``), so that every
        replay starts from the same addresses."""
        sim = self.ll_env._sim
        for fused in (_live(fused_pred), _live(fused_prey)):
            self._require_device_step_counter(fused)
        self._own_privileged()
        live, _, recurrent = self._who_acts(fused_pred, fused_prey)
        hold = recurrent and steps_per_replay % 2 == 1
        with_critic_memory = (with_critic_memory,) if isinstance(with_critic_memory, str) else tuple(with_critic_memory or ())

        def device_step():
            _, _, ll_actions, B = self._act(fused_pred, fused_prey, self.obs_buf_pred, self.obs_buf_prey, self.obs_buf_pred, self.obs_buf_prey, deterministic_pred,
                                            deterministic_prey, with_critic_memory=with_critic_memory,
                                            critic_obs={a: getattr(self, f"privileged_obs_buf_{a}") for a in AGENTS})
            if hold:
                live["pred"].hold_slot(); live["prey"].hold_slot()      # (a pool's state is its live actor's)
            sim.step(ll_actions, -1)
            self._post(B, -1, torch.cuda.current_stream(self.device).cuda_stream)
        self._policy_step_graph, replay = self._capture(device_step, warmup, steps_per_replay, self._step_result)
        self._policy_step_actors = (fused_pred, fused_prey)      # the graph reads their weights and memories where they are: they live as long as it does
        return replay

    # ------------------------------------------------------------------ resets and observations
    def reset_idx(self, env_ids):
        """Reset the listed envs from the host (reference :271-311): joints and root state of the prey, predator placement, history, counters,
        episode sums.  Resets that happen inside ``step`` are done by ``lg_dec_game_post`` with keyed Philox draws; this entry point serves
        ``reset()`` and tooling and draws from torch's generator, like the creation-time randomisation of the low-level env."""
        if len(env_ids) == 0:
            return
        ll = self.ll_env
        ids = torch.as_tensor(env_ids, device=self.device, dtype=torch.long)
        n = len(ids)
        ll.dof_pos[ids] = ll.default_dof_pos * (0.5 + torch.rand(n, ll.num_dof, device=self.device))     # low_level_game.py:391-392
        ll.dof_vel[ids] = 0.
        self._reset_roots(ids)
        self.obs_buf_prey[ids, 0:12] = self.MAX_REL_POS
        self.obs_buf_prey[ids, 12:16] = 0
        self.obs_buf_pred[ids] = -self.MAX_REL_POS
        self.episode_length_buf[ids] = 0
        self.reset_buf[ids] = True
        self.curr_episode_step[ids] = 0
        means = self._episode_sums[:, ids].mean(dim=1) / self.max_episode_length_s                        # (:298-305)
        self._episode_means.copy_(means)
        self._episode_sums[:, ids] = 0.
        if self._privileged:
            self._write_privileged()

    def reset(self):
        """Reset all envs, then one zero-command step (:313-319)."""
        self.reset_idx(torch.arange(self.num_envs, device=self.device))
        actions_pred = torch.zeros(self.num_envs, self.num_actions_pred, device=self.device, requires_grad=False)
        actions_prey = torch.zeros(self.num_envs, self.num_actions_prey, device=self.device, requires_grad=False)
        obs_pred, obs_prey, privileged_obs_pred, privileged_obs_prey, _, _, _, _ = self.step(actions_pred, actions_prey)
        return obs_pred, obs_prey, privileged_obs_pred, privileged_obs_prey

    def get_observations_pred(self):
        return self.obs_buf_pred

    def get_observations_prey(self):
        return self.obs_buf_prey

    def get_privileged_observations_pred(self):
        return self.privileged_obs_buf_pred

    def get_privileged_observations_prey(self):
        return self.privileged_obs_buf_prey

    def agent_view(self, agent, opponent):
        """The single-agent surface of ``agent`` ("pred" or "prey") with ``opponent`` -- a ``FusedActor`` or an ``rl.OpponentPool`` (device path)
        or a torch policy ``obs -> sampled actions`` (generic path) -- acting for the other agent inside every step."""
        return AgentView(self, agent, opponent)

    # ------------------------------------------------------------------ set-up
    def _init_buffers(self):
        N, dev = self.num_envs, self.device

        def prey_obs():
            t = self.MAX_REL_POS * torch.ones(N, self.num_obs_prey, device=dev, dtype=torch.float)
            t[:, 12:16] = 0                                                    # (:127-128)
            return t
        self._obs_pair_prey = (prey_obs(), prey_obs())
        self._obs_pair_pred = (self.MAX_REL_POS * torch.ones(N, self.num_obs_pred, device=dev, dtype=torch.float),
                               self.MAX_REL_POS * torch.ones(N, self.num_obs_pred, device=dev, dtype=torch.float))
        self._obs_flip = 0
        self.obs_buf_prey, self.obs_buf_pred = self._obs_pair_prey[0], self._obs_pair_pred[0]
        for a in self._privileged:                                            # written by lg_dec_game_privileged_obs before anyone reads them
            self._priv_pair[a] = tuple(torch.zeros(N, PRIVILEGED_WIDTHS[a], device=dev, dtype=torch.float) for _ in range(2))
        self._select_privileged()
        self.rew_buf_prey = torch.zeros(N, device=dev, dtype=torch.float)
        self.rew_buf_pred = torch.zeros(N, device=dev, dtype=torch.float)
        self.reset_buf = torch.ones(N, device=dev, dtype=torch.bool)          # persistent bool tensors, like the low-level env's (quirk Q1)
        self.time_out_buf = torch.zeros(N, device=dev, dtype=torch.bool)
        self.episode_length_buf = torch.zeros(N, device=dev, dtype=torch.long)
        self.curr_episode_step = torch.zeros(N, device=dev, dtype=torch.long)
        self.init_predator_pos = self._place_predator(self.ll_env.root_states[:, :3])
        self.predator_pos = self.init_predator_pos.clone()
        self._command_pred = torch.zeros(N, self.num_actions_pred, device=dev, dtype=torch.float)
        self._command_prey = torch.zeros(N, self.num_actions_prey, device=dev, dtype=torch.float)
        self._episode_sums = torch.zeros(len(SUMS), N, device=dev, dtype=torch.float)
        self._episode_means = torch.zeros(len(SUMS), device=dev, dtype=torch.float)
        self._extras_accum = torch.zeros(4, device=dev, dtype=torch.float)
        self._extras_ticket = torch.zeros(1, device=dev, dtype=torch.int32)
        if getattr(self.cfg.env, "send_timeouts", True):
            self.extras["time_outs"] = self.time_out_buf                      # this step's time-outs, refreshed by every lg_dec_game_post

    def _prepare_reward_functions(self):
        """Reference :527-579: zero scales dropped, the rest multiplied by the low-level dt; one episode sum per name, and
        ``extras["episode"]`` as views of the device episode means."""
        for scales in (self.reward_scales_prey, self.reward_scales_pred):
            for key in list(scales.keys()):
                if scales[key] == 0:
                    scales.pop(key)
                else:
                    scales[key] *= self.ll_env.dt
        if "termination" in self.reward_scales_pred:
            raise ValueError("rewards_predator.scales.termination is not supported: the reference reads a non-existent self.reward_scales for it "
                             "(dec_high_level_game.py:359) and raises at the first step")
        for who, scales, known in (("prey", self.reward_scales_prey, ("evasion", "termination")), ("pred", self.reward_scales_pred, ("pursuit",))):
            unknown = [k for k in scales if k not in known]
            if unknown:
                raise AttributeError(f"'DecHighLevelGame' object has no attribute '_reward_{unknown[0]}' ({who})")
        self.reward_names_prey = [k for k in self.reward_scales_prey if k != "termination"]
        self.reward_names_pred = list(self.reward_scales_pred)
        self.episode_sums_prey = {name: self._episode_sums[SUMS.index(name)] for name in self.reward_scales_prey}
        self.episode_sums_pred = {name: self._episode_sums[SUMS.index(name)] for name in self.reward_scales_pred}
        episode = {f"rew_pred_{name}": self._episode_means[SUMS.index(name)] for name in self.reward_scales_pred}
        episode.update({f"rew_prey_{name}": self._episode_means[SUMS.index(name)] for name in self.reward_scales_prey})
        self.extras["episode"] = episode

    def _parse_cfg(self, cfg):
        """Reference :581-590."""
        self.reward_scales_prey = class_to_dict(self.cfg.rewards_prey.scales)
        self.reward_scales_pred = class_to_dict(self.cfg.rewards_predator.scales)
        super()._parse_cfg(cfg)

    def _pack(self):
        """``lg_dec_game_params`` from the configs and the pointer table of ``lg_dec_game_buffers``."""
        ll, P = self.ll_env, capi.lg_dec_game_params()
        self._pack_common(P)
        P.only_positive_rewards_prey = int(bool(self.cfg.rewards_prey.only_positive_rewards))
        P.only_positive_rewards_pred = int(bool(self.cfg.rewards_predator.only_positive_rewards))
        P.max_episode_length, P.max_episode_length_s = int(self.max_episode_length), float(self.max_episode_length_s)
        P.scale_evasion_dt = float(self.reward_scales_prey.get("evasion", 0.0))
        P.scale_pursuit_dt = float(self.reward_scales_pred.get("pursuit", 0.0))
        P.scale_termination_prey_dt = float(self.reward_scales_prey.get("termination", 0.0))
        capi._fill(P.default_dof_pos, ll.default_dof_pos.cpu().numpy())        # the joint order of the low-level dof_state buffer
        self._P = P
        self._pointers = dict(self._ll_pointers(), ll_dof_state=ll._sim.buf["dof_state"].data_ptr(), predator_pos=self.predator_pos.data_ptr(),
                              rew_prey=self.rew_buf_prey.data_ptr(), rew_pred=self.rew_buf_pred.data_ptr(), reset_buf=self.reset_buf.data_ptr(),
                              time_out_buf=self.time_out_buf.data_ptr(), curr_episode_step=self.curr_episode_step.data_ptr(),
                              episode_length_buf=self.episode_length_buf.data_ptr(), episode_sums=self._episode_sums.data_ptr(),
                              episode_means=self._episode_means.data_ptr(), extras_accum=self._extras_accum.data_ptr(),
                              extras_ticket=self._extras_ticket.data_ptr())

    def set_command_ranges(self):
        """Re-pack after ``command_ranges`` / ``capture_dist`` were edited."""
        self._pack()

    def _bind(self, command_pred, command_prey, obs_pred, obs_prey):
        """``lg_dec_game_buffers`` for this call: the kernels read and clip the callers' tensors where they are."""
        command_pred = self._own(command_pred, self.num_actions_pred, self._command_pred, "command_pred")
        command_prey = self._own(command_prey, self.num_actions_prey, self._command_prey, "command_prey")
        self._keep = (command_pred, command_prey)
        return capi.dec_game_buffers(dict(self._pointers, command_pred=command_pred.detach().data_ptr(), command_prey=command_prey.detach().data_ptr(),
                                          obs_pred=obs_pred.data_ptr(), obs_prey=obs_prey.data_ptr()))


def _live(fused):
    """The ``FusedActor`` that supplies seed, step source and output buffers: ``fused`` itself, or the live member of an ``rl.OpponentPool``."""
    return fused.live if getattr(fused, "is_opponent_pool", False) else fused


class AgentView:
    """One agent of a ``DecHighLevelGame`` as a single-agent env: the surface ``rl.OnPolicyRunner`` drives for ``high_level_game``
    (``step`` on the generic path, ``step_policy`` on the device path).  The opponent produces the other agent's command inside every step
    and SAMPLES, like the learner; only this agent's transition is returned.  Both views of an env drive the same env."""
    dec_agent_view = True          # what the runner's time-out bootstrap of the device game rollout is guarded on

    def __init__(self, env, agent, opponent):
        if agent not in AGENTS:
            raise ValueError(f"agent must be one of {AGENTS}, got {agent!r}")
        self.env, self.agent, self.opponent = env, agent, opponent
        self.other = "prey" if agent == "pred" else "pred"
        self.num_envs, self.cfg, self.device, self.ll_env = env.num_envs, env.cfg, env.device, env.ll_env
        self.num_obs = getattr(env, f"num_obs_{agent}")
        self.num_actions = getattr(env, f"num_actions_{agent}")
        self.num_privileged_obs = getattr(env, f"num_privileged_obs_{agent}")
        self.max_episode_length = env.max_episode_length
        self.fused_seed_offset = SEED_OFFSET_PRED if agent == "pred" else SEED_OFFSET_PREY     # noise seed of this agent's FusedActor: cfg.seed + this

    # buffers are looked up at every access: the env alternates between two observation buffers per agent
    obs_buf = property(lambda self: getattr(self.env, f"obs_buf_{self.agent}"))
    rew_buf = property(lambda self: getattr(self.env, f"rew_buf_{self.agent}"))
    reset_buf = property(lambda self: self.env.reset_buf)
    extras = property(lambda self: self.env.extras)
    episode_length_buf = property(lambda self: self.env.episode_length_buf)
    dt = property(lambda self: self.env.dt)
    _obs_flip = property(lambda self: self.env._obs_flip)
    _capturing = property(lambda self: self.env._capturing)

    @property
    def common_step_counter(self):
        return self.env.common_step_counter

    @common_step_counter.setter
    def common_step_counter(self, value):
        self.env.common_step_counter = value

    def begin_graph_capture(self):
        self.env.begin_graph_capture()

    def capture_extras_flush(self):
        self.env.capture_extras_flush()

    def end_graph_capture(self, steps_captured):
        self.env.end_graph_capture(steps_captured)

    def capture_state(self):
        return self.env.capture_state()

    def abort_graph_capture(self, state):
        self.env.abort_graph_capture(state)

    def reset(self):
        obs_pred, obs_prey, priv_pred, priv_prey = self.env.reset()
        return (obs_pred, priv_pred) if self.agent == "pred" else (obs_prey, priv_prey)

    def get_observations(self):
        return self.obs_buf

    def get_privileged_observations(self):
        return getattr(self.env, f"privileged_obs_buf_{self.agent}")

    def refresh_privileged_observations(self):
        self.env.refresh_privileged_observations()

    def _result(self, out):
        obs_pred, obs_prey, priv_pred, priv_prey, rew_pred, rew_prey, dones, extras = out
        return (obs_pred, priv_pred, rew_pred, dones, extras) if self.agent == "pred" else (obs_prey, priv_prey, rew_prey, dones, extras)

    def step(self, actions):
        """Generic path: ``opponent`` is a torch policy ``obs -> sampled actions``.  ``actions`` is clipped in place, as by ``env.step``."""
        with torch.no_grad():
            other = self.opponent(getattr(self.env, f"obs_buf_{self.other}")).detach().clone()
        if self.agent == "pred":
            return self._result(self.env.step(actions, other))
        return self._result(self.env.step(other, actions))

    def step_policy(self, fused, deterministic=False, sample=None, sigma=None, log_prob=None, obs_copy=None, with_critic_memory=False, privileged_out=None):
        """Device path: ``opponent`` is a ``FusedActor`` or an ``rl.OpponentPool`` (a mixture of opponents by 32-env block).  Returns ``(command, mean), (obs, None, rew, dones, extras)`` of this agent, the
        contract of ``HighLevelGame.step_policy``.  Recurrent policies (``fused`` and ``opponent`` both ``RecurrentFusedActor`` s):
        ``with_critic_memory`` advances this agent's critic memory too and returns its output as a third value of the first tuple; of the
        opponent only the actor memory advances.  ``privileged_out``: a tensor for this agent's new privileged rows of the step (the
        env's ``step_policy``), returned in the result's second slot."""
        mine = {k: v for k, v in (("sample", sample), ("sigma", sigma), ("log_prob", log_prob), ("obs_copy", obs_copy)) if v is not None}
        critic = (self.agent,) if with_critic_memory else ()
        priv = None if privileged_out is None else {self.agent: privileged_out}
        if self.agent == "pred":
            pred, _, out = self.env.step_policy(fused, self.opponent, deterministic_pred=deterministic, out_pred=mine, with_critic_memory=critic, privileged_out=priv)
            return pred, self._result(out)
        _, prey, out = self.env.step_policy(self.opponent, fused, deterministic_prey=deterministic, out_prey=mine, with_critic_memory=critic, privileged_out=priv)
        return prey, self._result(out)

    def shared_actor_launch(self, fused):
        """``DecHighLevelGame.shared_actor_launch`` with the opponent; None while the view has no opponent yet (``DecGamePolicyRunner`` sets
        it once both agents' actors exist and makes the call then)."""
        if self.opponent is None:
            return None
        return self.env.shared_actor_launch(fused, self.opponent) if self.agent == "pred" else self.env.shared_actor_launch(self.opponent, fused)
