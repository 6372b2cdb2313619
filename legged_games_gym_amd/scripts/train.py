"""CLI entry point (reference ``legged_gym/scripts/train.py:39-47``):
``python -m legged_games_gym_amd.scripts.train --task=anymal_c_flat --headless``

Multi-GPU (new, the reference is single-process): launch one process per GPU,
``python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 -m legged_games_gym_amd.scripts.train
--task=anymal_c_rough --headless``.  Every rank owns its own ``num_envs`` environments on ``cuda:LOCAL_RANK`` (env seed
= registered seed + rank), the policy is replicated (rank 0's initial weights are broadcast) and kept identical by the
collectives of ``rl/ppo.py`` (RCCL: all-gather of returns/advantages, gradient and mean-KL all-reduce); only rank 0 writes logs
and checkpoints.

``--task=high_level_game --device_rollout`` trains the game on its device path: the high-level actor on the matrix cores, three launches
per step, the whole rollout one graph replay (off by default: the generic VecEnv loop).  ``--task=scripted_predator_game`` trains the prey
alone against the reference's scripted pursuer, on either path.  ``--outcome_stats`` (both game tasks, either path) logs who wins: the
shares of finished episodes that ended in a capture, outside the arena, with a fallen robot or with the prey surviving, and their mean
length, as ``Episode/outcome_*``.

``--policy_class_name ActorCriticRecurrent [--rnn_type lstm --rnn_hidden_size 256 --rnn_num_layers 1]`` trains an LSTM policy (rsl_rl's class
of that name): on a locomotion task on the GPU the memories and the actor run on the device in the rollout (``lg_lstm_step``), the update is
back-propagation through time in torch; ``high_level_game`` / ``scripted_predator_game`` take the generic loop, or with ``--device_rollout`` four
launches per step (``lg_lstm_step`` -> ``lg_game_lstm_act`` -> ``lg_step`` -> the post kernel), the rollout one graph replay.  ``--device_bptt`` (off by default) moves the recurrence of
that update onto the device as well: both memories' padded trajectories run through time in ``lg_lstm_seq_forward`` / ``lg_lstm_seq_backward``
(one launch each way per memory and mini-batch); the MLPs, the loss and Adam stay in torch."""
import os

from legged_games_gym_amd.envs import *  # noqa: F401,F403  (registers the locomotion tasks)
from legged_games_gym_amd.envs import a1_game
from legged_games_gym_amd.utils import get_args
from legged_games_gym_amd.utils.helpers import apply_policy_args
from legged_games_gym_amd.utils.task_registry import task_registry


def _init_distributed(args):
    """torchrun / torch.distributed.run environment -> process group, per-rank device, per-rank env seed."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1:
        return 0, 1
    import torch
    import torch.distributed as dist
    rank = int(os.environ["RANK"])
    local = int(os.environ.get("LG_LOCAL_DEVICE", os.environ.get("LOCAL_RANK", "0")))     # LG_LOCAL_DEVICE: rehearsal of N ranks on one GPU
    on_gpu = torch.cuda.is_available() and not str(args.rl_device).startswith("cpu")
    if on_gpu:
        torch.cuda.set_device(local)
        args.sim_device = args.rl_device = f"cuda:{local}"
        args.sim_device_id = local
    dist.init_process_group(backend=os.environ.get("LG_DIST_BACKEND", "nccl" if on_gpu else "gloo"))      # "nccl" is RCCL on ROCm
    _, train_cfg = task_registry.get_cfgs(args.task)
    train_cfg.seed = int(train_cfg.seed) + rank          # the env seeds from the registered train cfg (reference quirk Q10)
    return rank, world


def train(args):
    if args.task in a1_game.DEC_TASKS:
        raise SystemExit(f"--task={args.task} trains two policies in alternation: use python -m legged_games_gym_amd.scripts.train_dec_game --task={args.task}")
    if args.task in a1_game.TASKS:
        a1_game.register()               # the game layer registers on demand: python -m legged_games_gym_amd.scripts.train --task=high_level_game --headless
    if args.task in a1_game.SCRIPTED_TASKS:
        a1_game.register_scripted()      # python -m legged_games_gym_amd.scripts.train --task=scripted_predator_game --headless [--device_rollout]
    rank, world = _init_distributed(args)
    if args.device_rollout:                  # a runner key, read with .get(): the config classes stay value for value the reference's
        task_registry.get_cfgs(args.task)[1].runner.device_rollout = True
    if args.device_bptt:                     # likewise a runner key
        task_registry.get_cfgs(args.task)[1].runner.device_bptt = True
    if args.wide_memory:                     # likewise: memories of up to 512 units on the device rollout
        task_registry.get_cfgs(args.task)[1].runner.wide_memory = True
    if args.device_gru:                      # likewise: GRU memories on the device rollout
        task_registry.get_cfgs(args.task)[1].runner.device_gru = True
    apply_policy_args(task_registry.get_cfgs(args.task)[1], args)     # --policy_class_name ActorCriticRecurrent [--rnn_type / --rnn_hidden_size / --rnn_num_layers]
    if args.outcome_stats:                   # read with getattr() by the game tasks: no field of the registered config classes
        if args.task not in a1_game.TASKS + a1_game.SCRIPTED_TASKS:
            raise SystemExit(f"--outcome_stats is for {', '.join(a1_game.TASKS + a1_game.SCRIPTED_TASKS)}, not --task={args.task}")
        task_registry.get_cfgs(args.task)[0].env.outcome_stats = True
    env, env_cfg = task_registry.make_env(name=args.task, args=args)
    ppo_runner, train_cfg = task_registry.make_alg_runner(env=env, name=args.task, args=args, **({} if rank == 0 else {"log_root": None}))
    ppo_runner.learn(num_learning_iterations=train_cfg.runner.max_iterations, init_at_random_ep_len=True)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    train(get_args())
