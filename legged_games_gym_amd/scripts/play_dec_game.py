"""Headless evaluation of the decentralised predator-prey game (the in-scope part of reference ``legged_gym/scripts/play_dec_game.py``):
the newest ``dec_high_level_game`` checkpoint is loaded and both agents' inference policies step the env.
``python -m legged_games_gym_amd.scripts.play_dec_game --task=dec_high_level_game --headless``"""
import torch

from legged_games_gym_amd.envs import *  # noqa: F401,F403
from legged_games_gym_amd.envs import a1_game
from legged_games_gym_amd.utils.task_registry import task_registry

from .train_dec_game import _args


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
    env, _ = task_registry.make_env(name=args.task, args=args, env_cfg=env_cfg)
    train_cfg.runner.resume = True
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


if __name__ == "__main__":
    play(_args())
