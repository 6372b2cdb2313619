"""Headless evaluation of a trained game policy (the in-scope part of reference ``legged_gym/scripts/play_game.py``): who wins?

``python -m legged_games_gym_amd.scripts.play_game --task={high_level_game,scripted_predator_game} --headless
[--load_run RUN --checkpoint K --num_envs N --steps S]``

The newest checkpoint of the task is loaded through the runner, as ``scripts/play.py`` does; the outcome statistics of the env are switched
on (include/legged_game_outcome.h) and ``S`` high-level steps (default: 2 x ``max_episode_length``) are rolled out with the deterministic
policy -- as replays of the graphed three-launch policy step where ``lg_game_act`` has a kernel for the actor pair (four launches with a
recurrent checkpoint, ``--policy_class_name ActorCriticRecurrent`` and the ``--rnn_*`` flags it was trained with: ``lg_lstm_step`` and
``lg_game_lstm_act`` in front), else through ``step()`` with the runner's inference policy.  The totals are read ONCE, at the end.  A table is printed and ``outcomes_<iteration>.json`` is written
next to the checkpoint: ``totals`` (the seven integers of ``env.outcome_totals()``; its ``steps`` is the summed length of the finished
episodes), ``rates`` (the five flags over ``episodes``), ``mean_steps``, ``num_envs`` and ``steps`` (the ``S`` of the rollout).

Episodes still running when the rollout ends are NOT counted, which favours short episodes: with few steps the capture rate is overstated
and the survival rate understated.  The flags are not exclusive (an env may be captured in the step its low-level episode runs out), so
the rates need not add up to one.  The reference's viewer, camera motion, frame recording and goal-reaching branch are out of scope."""
import json
import os

import torch

import legged_games_gym_amd.utils.task_registry as registry_module
from legged_games_gym_amd.envs import *  # noqa: F401,F403
from legged_games_gym_amd.envs import a1_game
from legged_games_gym_amd.utils import get_args
from legged_games_gym_amd.utils.helpers import apply_policy_args, get_load_path
from legged_games_gym_amd.utils.task_registry import task_registry

COUNTS = ("episodes", "captured", "prey_out", "predator_out", "fell", "survived", "steps")
FLAGS = COUNTS[1:6]


def outcome_rates(totals):
    """``totals``: the seven integers of ``env.outcome_totals()`` -> ``{"<flag>_rate": flag / episodes for the five flags, "mean_steps":
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


def play_game(args, steps=None):
    """-> (env, result dict as written to the JSON file, path of the file)."""
    if args.task not in a1_game.TASKS + a1_game.SCRIPTED_TASKS:
        raise SystemExit(f"play_game plays {a1_game.TASKS + a1_game.SCRIPTED_TASKS}; --task={args.task} is not one of them")
    if args.task in a1_game.TASKS:
        a1_game.register()
    if args.task in a1_game.SCRIPTED_TASKS:
        a1_game.register_scripted()
    env_cfg, train_cfg = task_registry.get_cfgs(name=args.task)
    env_cfg.terrain.num_rows = 5
    env_cfg.terrain.num_cols = 5
    env_cfg.terrain.curriculum = False
    env_cfg.noise.add_noise = False
    env_cfg.domain_rand.randomize_friction = False
    env_cfg.domain_rand.push_robots = False
    env, _ = task_registry.make_env(name=args.task, args=args, env_cfg=env_cfg)
    train_cfg.runner.resume = True
    apply_policy_args(train_cfg, args)      # --policy_class_name ActorCriticRecurrent [--rnn_*]: the flags the checkpoint was trained with
    runner, train_cfg = task_registry.make_alg_runner(env=env, name=args.task, args=args, train_cfg=train_cfg)
    log_root = os.path.join(registry_module.LEGGED_GYM_ROOT_DIR, "logs", train_cfg.runner.experiment_name)
    checkpoint = get_load_path(log_root, load_run=train_cfg.runner.load_run, checkpoint=train_cfg.runner.checkpoint)
    iteration = int(runner.current_learning_iteration)

    env.enable_outcome_stats()              # before the capture below: a graph keeps the launch the switch selected when it was captured
    n = int(steps) if steps is not None else 2 * int(env.max_episode_length)
    replay = None
    if str(env.device).startswith("cuda"):
        from legged_games_gym_amd.rl import FusedActor
        try:
            ac, kw = runner.alg.actor_critic, dict(seed=int(getattr(env.cfg, "seed", 1)), step_counter=env.ll_env._sim.buf["step_counter"])
            if ac.is_recurrent:             # memories from zero, lg_lstm_step -> lg_game_lstm_act -> lg_step -> post per step
                from legged_games_gym_amd.rl.recurrent_actor import RecurrentFusedActor
                fused = RecurrentFusedActor(ac, env.device, num_envs=env.num_envs, wide=getattr(args, "wide_memory", False),
                                            gru=getattr(args, "device_gru", False), **kw)
            else:
                fused = FusedActor(ac, env.device, **kw)
            if env.shared_actor_launch(fused) or getattr(fused, "wide", False):     # (a wide memory: the graph holds the separate launches)
                with torch.inference_mode():        # as the runner captures its rollouts: torch's per-capture generator state may stem from such a capture
                    replay = env.make_graphed_policy_step(fused, deterministic=True)
        except ValueError as exc:           # an actor the MFMA kernels have no shape for
            print(f"[play_game] device policy step unavailable ({exc}); stepping through the inference policy")
    env.reset_outcome_totals()              # (the capture's warm-up steps are not part of the evaluation)
    with torch.inference_mode():
        if replay is not None:
            path_used = "graphed policy step"
            for _ in range(n):
                replay()
        else:
            path_used = "step() with the inference policy"
            policy = runner.get_inference_policy(device=env.device)
            obs = env.get_observations()
            for _ in range(n):
                obs, _, _, _, _ = env.step(policy(obs.detach()).detach().clone())
    totals = env.outcome_totals()           # the one synchronising read
    rates = outcome_rates(totals)
    clean = {k: (v if v == v else None) for k, v in rates.items()}                     # no finished episode: null, not NaN, in the file
    result = dict(task=args.task, iteration=iteration, num_envs=int(env.num_envs), steps=n, path=path_used, totals={k: int(totals[k]) for k in COUNTS},
                  rates={k: clean[k] for k in clean if k != "mean_steps"}, mean_steps=clean["mean_steps"])
    print(format_table(totals, rates, env.num_envs, n))
    out = os.path.join(os.path.dirname(checkpoint), f"outcomes_{iteration}.json")
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print("written to:", out)
    return env, result, out


def _args(argv=None):
    import argparse
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument("--steps", type=int, default=None, help="high-level steps to roll out (default: 2 x max_episode_length)")
    own, rest = pre.parse_known_args(argv)
    args = get_args(rest)
    args.steps = own.steps
    return args


if __name__ == "__main__":
    _a = _args()
    play_game(_a, steps=_a.steps)
