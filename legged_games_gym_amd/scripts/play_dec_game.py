"""Headless evaluation of the decentralised predator-prey game (the in-scope part of reference ``legged_gym/scripts/play_dec_game.py``):
the newest ``dec_high_level_game`` checkpoint is loaded and both agents' inference policies step the env.
``python -m legged_games_gym_amd.scripts.play_dec_game --task=dec_high_level_game --headless``

``--outcomes [--load_run RUN --checkpoint K --num_envs N --steps S]`` answers "who wins?" instead (``play_outcomes``): the outcome statistics
of the env are switched on (include/legged_dec_game_outcome.h) and ``S`` high-level steps (default: 2 x ``max_episode_length``) are rolled
out with BOTH agents deterministic -- as replays of the graphed three-launch policy step where ``lg_dec_game_act`` has a kernel for the actor
triple, else through ``step_policy`` (separate actor launches), else through ``step`` with the runner's inference policies.  The totals are
read ONCE, at the end.  A recurrent checkpoint (``--policy_class_name ActorCriticRecurrent`` and the ``--rnn_*`` flags it was trained with) goes
through the graphed policy step as well: ``lg_dec_lstm_step`` with the two actor memories only, starting from zero states, then
``lg_dec_game_lstm_act``.  A table is printed and ``outcomes_<iteration>.json`` is written next to the checkpoint: ``totals`` (the six
integers of ``env.outcome_totals()``; its ``steps`` is the summed length of the finished episodes), ``rates`` (the four flags over
``episodes``), ``mean_steps``, ``num_envs``, ``steps`` (the ``S`` of the rollout), ``task``, ``iteration`` and ``path``.

Episodes still running when the rollout ends are NOT counted, which favours short episodes: with few steps the capture rate is overstated.
The flags are not exclusive (an env may be captured in the step its low-level episode runs out), so the rates need not add up to one.
``--privileged_critic {prey,pred,both}``: the flag the checkpoint was trained with; only the critic's shape depends on it, and a checkpoint
whose critic has another input width is refused with an error that names the flag.
``DecEvaluation`` is what ``play_outcomes`` and ``scripts/crossplay_dec_game.py`` share."""
import copy
import json
import os

import torch

from legged_games_gym_amd.envs import *  # noqa: F401,F403
import legged_games_gym_amd.utils.task_registry as registry_module
from legged_games_gym_amd.envs import a1_game
from legged_games_gym_amd.utils.helpers import apply_policy_args, get_load_path
from legged_games_gym_amd.utils.task_registry import task_registry

from .train_dec_game import _args as _train_args

COUNTS = ("episodes", "captured", "timed_out", "fell", "ll_timed_out", "steps")
FLAGS = COUNTS[1:5]


def play(args, steps=None):
    if args.task not in a1_game.DEC_TASKS:
        raise SystemExit(f"play_dec_game plays {a1_game.DEC_TASKS}; use scripts.play for --task={args.task}")
    a1_game.register_dec()
    env_cfg, train_cfg = task_registry.get_cfgs(name=args.task)
    env_cfg.env.num_envs = min(env_cfg.env.num_envs, 50)
    env_cfg.terrain.num_rows = 5
    env_cfg.terrain.num_cols = 5
    env_cfg.terrain.curriculum = False
    env_cfg.noise.add_noise = False
    env_cfg.domain_rand.randomize_friction = False
    env_cfg.domain_rand.push_robots = False
    a1_game.set_privileged_critic(env_cfg, getattr(args, "privileged_critic", None))     # only to rebuild a critic of the checkpoint's shape
    env, _ = task_registry.make_env(name=args.task, args=args, env_cfg=env_cfg)
    train_cfg.runner.resume = True
    apply_policy_args(train_cfg, args)
    if getattr(train_cfg.runner, "policy_class_name", "ActorCritic") == "ActorCriticRecurrent":
        train_cfg.runner.device_rollout = True      # what the runner builds two recurrent policies for
    runner, train_cfg = task_registry.make_dec_alg_runner(env=env, name=args.task, args=args, train_cfg=train_cfg, log_root="default")
    policy_pred = runner.get_inference_policy("pred", device=env.device)
    policy_prey = runner.get_inference_policy("prey", device=env.device)
    obs_pred, obs_prey = env.get_observations_pred(), env.get_observations_prey()
    n = steps if steps is not None else 10 * int(env.max_episode_length)
    tot_pred, tot_prey = torch.zeros(env.num_envs, device=env.device), torch.zeros(env.num_envs, device=env.device)
    captures = 0
    for _ in range(n):
        with torch.no_grad():
            a_pred, a_prey = policy_pred(obs_pred.detach()), policy_prey(obs_prey.detach())
        obs_pred, obs_prey, _, _, rew_pred, rew_prey, dones, _ = env.step(a_pred.detach().clone(), a_prey.detach().clone())
        tot_pred += rew_pred
        tot_prey += rew_prey
        captures += int((dones & ~env.time_out_buf & ~env.ll_env.reset_buf).sum())
    print(f"{n} steps: mean reward per step predator {(tot_pred / n).mean().item():.4f}, prey {(tot_prey / n).mean().item():.4f}; {captures} captures")
    return env


def dec_outcome_rates(totals):
    """``totals``: the six integers of ``env.outcome_totals()`` -> ``{"<flag>_rate": flag / episodes for the four flags, "mean_steps":
    steps / episodes}``, in Python floats; every value is NaN when no episode finished."""
    n = int(totals["episodes"])
    out = {f"{k}_rate": (int(totals[k]) / n if n > 0 else float("nan")) for k in FLAGS}
    out["mean_steps"] = int(totals["steps"]) / n if n > 0 else float("nan")
    return out


def format_table(totals, rates, num_envs, steps):
    lines = [f"{num_envs} envs x {steps} high-level steps: {int(totals['episodes'])} finished episodes", f"{'outcome':<14}{'episodes':>10}{'rate':>9}"]
    lines += [f"{k:<14}{int(totals[k]):>10}{rates[k + '_rate']:>9.3f}" for k in FLAGS]
    lines.append(f"mean episode length {rates['mean_steps']:.1f} high-level steps")
    lines.append("episodes still running at the end are not counted, which favours short episodes; an episode may raise several outcomes")
    return "\n".join(lines)


class DecEvaluation:
    """One env, one pair of device actors and one deterministic step path of ``dec_high_level_game`` for evaluation rollouts that all begin
    at the SAME start: ``torch.manual_seed(seed)``, ``env.reset()``, and a copy of everything on the device taken right there, which
    ``run`` puts back -- with the low-level step counter, which keys every reset draw -- before it rolls out.  On the device path the step is
    captured ONCE; ``load`` swaps weights underneath the graph (``FusedActor.sync_device`` repacks in place; for a recurrent run
    ``RecurrentFusedActor.sync_device`` repacks both memories and the actor), and ``run`` starts all memories from zero, so a cell never meets
    the state another pair of policies left."""
    ENV_STATE = ("rew_buf_prey", "rew_buf_pred", "reset_buf", "time_out_buf", "episode_length_buf", "curr_episode_step", "predator_pos", "_episode_sums",
                 "_episode_means", "_extras_accum", "_extras_ticket")

    def __init__(self, args):
        if args.task not in a1_game.DEC_TASKS:
            raise SystemExit(f"play_dec_game plays {a1_game.DEC_TASKS}; use scripts.play_game for --task={args.task}")
        a1_game.register_dec()
        env_cfg, train_cfg = task_registry.get_cfgs(name=args.task)
        env_cfg, train_cfg = copy.deepcopy(env_cfg), copy.deepcopy(train_cfg)      # the registered objects keep their values (--num_envs lands on a copy)
        env_cfg.terrain.num_rows = 5
        env_cfg.terrain.num_cols = 5
        env_cfg.terrain.curriculum = False
        env_cfg.noise.add_noise = False
        env_cfg.domain_rand.randomize_friction = False
        env_cfg.domain_rand.push_robots = False
        a1_game.set_privileged_critic(env_cfg, getattr(args, "privileged_critic", None))     # only to rebuild a critic of the checkpoint's shape
        env, _ = task_registry.make_env(name=args.task, args=args, env_cfg=env_cfg)
        train_cfg.runner.resume = True
        for key in ("device_rollout", "graphed_rollout"):        # the runner only holds the two ActorCritics here
            if hasattr(train_cfg.runner, key):
                delattr(train_cfg.runner, key)
        apply_policy_args(train_cfg, args)      # --policy_class_name ActorCriticRecurrent [--rnn_*]: the flags the checkpoint was trained with
        self.recurrent = getattr(train_cfg.runner, "policy_class_name", "ActorCritic") == "ActorCriticRecurrent"
        if self.recurrent:                      # ... and the two RecurrentFusedActors: the runner builds them on the device path only
            train_cfg.runner.device_rollout, train_cfg.runner.graphed_rollout = True, False
            if getattr(args, "wide_memory", False):      # memories of up to 512 units, as the run was trained
                train_cfg.runner.wide_memory = True
            if getattr(args, "device_gru", False):       # GRU memories on the device, as the run was trained
                train_cfg.runner.device_gru = True
            if getattr(args, "dec_gru_shared", False):   # ... on the two shared launches (on top of device_gru)
                train_cfg.runner.dec_gru_shared = True
        runner, train_cfg = task_registry.make_dec_alg_runner(env=env, name=args.task, args=args, train_cfg=train_cfg, log_root=None)
        log_root = os.path.join(registry_module.LEGGED_GYM_ROOT_DIR, "logs", train_cfg.runner.experiment_name)
        self.checkpoint = get_load_path(log_root, load_run=train_cfg.runner.load_run, checkpoint=train_cfg.runner.checkpoint)
        self.env, self.runner, self.task = env, runner, args.task
        self.iteration = int(runner.current_learning_iteration)
        self.modules = {a: runner.runners[a].alg.actor_critic for a in ("pred", "prey")}
        self.seed = int(getattr(env.cfg, "seed", 1) or 1)

        env.enable_outcome_stats()              # before the capture below: a graph keeps the launch the switch selected when it was captured
        torch.manual_seed(self.seed)            # reset_idx from the host draws from torch's generator
        env.reset()
        self._start = self._snapshot()
        self.fused, self._replay, self.path = None, None, "step() with the inference policies"
        if self.recurrent:                      # the runners' own actors: on the device step counter, seeds apart
            self.fused = {a: runner.runners[a]._fused for a in ("pred", "prey")}
        elif str(env.device).startswith("cuda"):
            from legged_games_gym_amd.envs.a1_game.dec_high_level_game import SEED_OFFSET_PRED, SEED_OFFSET_PREY
            from legged_games_gym_amd.rl import FusedActor
            try:
                ctr = env.ll_env._sim.buf["step_counter"]
                self.fused = {"pred": FusedActor(self.modules["pred"], env.device, seed=self.seed + SEED_OFFSET_PRED, step_counter=ctr),
                              "prey": FusedActor(self.modules["prey"], env.device, seed=self.seed + SEED_OFFSET_PREY, step_counter=ctr)}
            except ValueError as exc:           # an actor the MFMA kernels have no shape for
                print(f"[play_dec_game] device policy step unavailable ({exc}); stepping through the inference policies")
        if self.fused is not None:
            env.ll_env._sim.buf["step_counter"].fill_(env.ll_env.common_step_counter)
            env.step_policy(self.fused["pred"], self.fused["prey"], deterministic_pred=True, deterministic_prey=True)      # does the triple have the shared launch?
            if env.last_act_rc == 0:
                self._restore()
                self._replay = env.make_graphed_policy_step(self.fused["pred"], self.fused["prey"], deterministic_pred=True, deterministic_prey=True)
                self.path = "graphed policy step"
            else:
                self.path = "step_policy() with separate actor launches"

    def _snapshot(self):
        env, ll = self.env, self.env.ll_env
        return dict(sim={k: v.clone() for k, v in ll._sim.buf.items() if torch.is_tensor(v)}, env={k: getattr(env, k).clone() for k in self.ENV_STATE},
                    obs=(env.obs_buf_pred.clone(), env.obs_buf_prey.clone(), ll.obs_buf.clone()), counter=int(ll.common_step_counter))

    def _restore(self):
        env, ll, snap = self.env, self.env.ll_env, self._start
        for k, v in snap["sim"].items():
            ll._sim.buf[k].copy_(v)
        for k, v in snap["env"].items():
            getattr(env, k).copy_(v)
        for t, v in zip((env.obs_buf_pred, env.obs_buf_prey, ll.obs_buf), snap["obs"]):     # the CURRENT buffer of each ping-pong pair
            t.copy_(v)
        ll.common_step_counter = snap["counter"]
        ll._sim.buf["step_counter"].fill_(snap["counter"])
        if self.recurrent and self.fused is not None:
            for fused in self.fused.values():   # memories start from zero
                fused.reset_states()

    def load(self, state_pred, state_prey):
        """Put the ``model_state_dict`` halves of two checkpoints under the step path (the captured graph is NOT re-captured): both
        ``FusedActor`` s, or both ``RecurrentFusedActor`` s, are repacked in place."""
        from legged_games_gym_amd.rl.runner import check_critic_width
        for a, state in (("pred", state_pred), ("prey", state_prey)):
            check_critic_width(self.modules[a], state, a)
        self.modules["pred"].load_state_dict(state_pred)
        self.modules["prey"].load_state_dict(state_prey)
        if self.fused is not None:
            self.fused["pred"].sync_device()
            self.fused["prey"].sync_device()

    def run(self, steps):
        """From the start state: zero the totals, ``steps`` deterministic steps, -> ``env.outcome_totals()`` (the one synchronising read)."""
        env = self.env
        with torch.inference_mode():
            self._restore()
            env.reset_outcome_totals()
            if self._replay is not None:
                for _ in range(steps):
                    self._replay()
            elif self.fused is not None:
                for _ in range(steps):
                    env.step_policy(self.fused["pred"], self.fused["prey"], deterministic_pred=True, deterministic_prey=True)
            else:
                for _ in range(steps):
                    a_pred, a_prey = self.modules["pred"].act_inference(env.obs_buf_pred), self.modules["prey"].act_inference(env.obs_buf_prey)
                    env.step(a_pred.detach().clone(), a_prey.detach().clone())
        return env.outcome_totals()


def result_of(totals):
    """``totals`` -> (rates with NaN, the JSON-clean pieces ``totals``, ``rates``, ``mean_steps``: null, not NaN, when no episode finished)."""
    rates = dec_outcome_rates(totals)
    clean = {k: (v if v == v else None) for k, v in rates.items()}
    return rates, dict(totals={k: int(totals[k]) for k in COUNTS}, rates={k: clean[k] for k in clean if k != "mean_steps"}, mean_steps=clean["mean_steps"])


def play_outcomes(args, steps=None):
    """-> (env, result dict as written to the JSON file, path of the file)."""
    ev = DecEvaluation(args)
    env = ev.env
    n = int(steps) if steps is not None else 2 * int(env.max_episode_length)
    totals = ev.run(n)
    rates, pieces = result_of(totals)
    result = dict(task=args.task, iteration=ev.iteration, num_envs=int(env.num_envs), steps=n, path=ev.path, **pieces)
    print(format_table(totals, rates, env.num_envs, n))
    out = os.path.join(os.path.dirname(ev.checkpoint), f"outcomes_{ev.iteration}.json")
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print("written to:", out)
    return env, result, out


def _args(argv=None):
    import argparse
    import sys
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument("--steps", type=int, default=None, help="high-level steps to roll out (default: 2 x max_episode_length with --outcomes)")
    pre.add_argument("--outcomes", action="store_true", default=False, help="count the outcomes of a deterministic rollout and write outcomes_<iteration>.json")
    own, rest = pre.parse_known_args(list(sys.argv[1:] if argv is None else argv))
    args = _train_args(rest)
    args.steps, args.outcomes = own.steps, own.outcomes
    return args


if __name__ == "__main__":
    _a = _args()
    if _a.outcomes:
        play_outcomes(_a, steps=_a.steps)
    else:
        play(_a, steps=_a.steps)
