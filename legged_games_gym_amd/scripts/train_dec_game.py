"""CLI entry point of the decentralised predator-prey game (reference ``legged_gym/scripts/train_dec_game.py``):
``python -m legged_games_gym_amd.scripts.train_dec_game --task=dec_high_level_game --headless``

Predator and prey are trained in alternating evolutions (``rl.DecGamePolicyRunner``): ``--max_evolutions`` evolutions of
``--max_iterations`` PPO iterations each (defaults: the registered train cfg's ``runner.max_evolutions`` / ``runner.max_iterations``).
``--device_rollout`` trains on the device path: both agents' actors on the matrix cores, three launches per step, every rollout one graph
replay (off by default: the generic VecEnv loop).  ``--outcome_stats`` (either path) logs who wins: the shares of captures, game time-outs,
falls and low-level time-outs among the finished episodes and their mean length, as ``Episode/outcome_*`` of both agents' tables.
``--opponent_pool K [--opponent_latest_share F]`` (device path only) lets the opponent of the learning agent be a mixture: the live opponent
in the share F (default 0.5) of the 32-env blocks, up to K frozen earlier versions of it in the rest (``rl.OpponentPool``);
the checkpoints then carry the pools.  With ``--outcome_stats`` as well, the outcomes are also counted per pool member and logged to
``opponents.csv``, and ``--opponent_priority P`` (P > 0) deals the non-live blocks by prioritised fictitious self-play: a past opponent the
learner loses to gets more envs.  ``--policy_class_name ActorCriticRecurrent [--rnn_hidden_size H]`` with ``--device_rollout``
trains two LSTM policies (four launches per step: ``lg_dec_lstm_step`` -> ``lg_dec_game_lstm_act`` -> ``lg_step`` -> post); without
``--device_rollout``, on the CPU, with a GRU / several layers / more than 256 units or with ``--opponent_pool`` alone the runner stops and says
why.  ``--wide_memory`` runs memories of 288 .. 512 units (the reference's ``rnn_hidden_size = 512``) on the kernels of liblegged_lstm_wide.so with
separate launches per step; not together with ``--opponent_pool_recurrent``.  ``--rnn_type gru --device_gru`` trains two GRU policies
(one layer, up to 256 units) on the cell of liblegged_gru.so, with separate launches per step as well; not together with
``--opponent_pool_recurrent`` either; ``--dec_gru_shared`` on top of it takes the two shared launches (``lg_dec_gru_step`` of
liblegged_dec_game_gru.so -> ``lg_dec_game_lstm_act``).  ``--opponent_pool K --opponent_pool_recurrent`` gives two recurrent policies their pools (``rl.RecurrentOpponentPool``: the launches are
``lg_dec_pool_lstm_step`` -> ``lg_dec_pool_lstm_act``, the weights of a block's actor memory and actor MLP its pool member's).
``--privileged_critic {prey,pred,both}`` gives that agent an asymmetric critic: it reads the true relative position, the prey's heading and
the episode clock (the predator's: the prey's velocity and whether the prey sees it), written by one more launch per step,
``lg_dec_game_privileged_obs``; the actor keeps the sensor's view.  The play scripts take the same flag to rebuild the critic.
Needs a trained ``a1`` checkpoint, like ``high_level_game``."""
from legged_games_gym_amd.envs import *  # noqa: F401,F403  (registers the locomotion tasks)
from legged_games_gym_amd.envs import a1_game
from legged_games_gym_amd.utils import get_args
from legged_games_gym_amd.utils.helpers import apply_policy_args
from legged_games_gym_amd.utils.task_registry import task_registry

DEFAULT_TASK = "dec_high_level_game"


def train(args):
    if args.task not in a1_game.DEC_TASKS:
        raise SystemExit(f"train_dec_game trains {a1_game.DEC_TASKS}; use scripts.train for --task={args.task}")
    a1_game.register_dec()
    apply_policy_args(task_registry.get_cfgs(args.task)[1], args)     # --policy_class_name ActorCriticRecurrent [--rnn_type / --rnn_hidden_size / --rnn_num_layers]
    if args.device_rollout:                  # a runner key, read with .get(): the config classes stay value for value the reference's
        task_registry.get_cfgs(args.task)[1].runner.device_rollout = True
    if args.wide_memory:                     # a runner key as well: memories of up to 512 units (separate launches, liblegged_lstm_wide.so)
        task_registry.get_cfgs(args.task)[1].runner.wide_memory = True
    if args.device_gru:                      # a runner key as well: GRU memories (--rnn_type gru; separate launches, liblegged_gru.so)
        task_registry.get_cfgs(args.task)[1].runner.device_gru = True
    if args.dec_gru_shared:                  # a runner key on top of device_gru: the GRU pair on the two shared launches (liblegged_dec_game_gru.so)
        task_registry.get_cfgs(args.task)[1].runner.dec_gru_shared = True
    if args.opponent_pool:                   # runner keys, read with .get() as well
        runner_cfg = task_registry.get_cfgs(args.task)[1].runner
        runner_cfg.opponent_pool_size, runner_cfg.opponent_latest_share = args.opponent_pool, args.opponent_latest_share
    if args.opponent_pool_recurrent:         # a runner key as well; the runner refuses it without the pool or with feed-forward policies
        task_registry.get_cfgs(args.task)[1].runner.opponent_pool_recurrent = True
    if args.opponent_priority:               # a runner key as well; the runner refuses it without the pool or the outcome statistics
        task_registry.get_cfgs(args.task)[1].runner.opponent_priority = args.opponent_priority
    if args.outcome_stats:                   # read with getattr() by the env: no field of the registered config classes
        task_registry.get_cfgs(args.task)[0].env.outcome_stats = True
    a1_game.set_privileged_critic(task_registry.get_cfgs(args.task)[0], getattr(args, "privileged_critic", None))     # before the env is made
    env, env_cfg = task_registry.make_env(name=args.task, args=args)
    runner, train_cfg = task_registry.make_dec_alg_runner(env=env, name=args.task, args=args)
    runner.learn(max_num_evolutions=train_cfg.runner.max_evolutions, num_learning_iterations=train_cfg.runner.max_iterations, init_at_random_ep_len=True)
    return runner


def _args(argv=None):
    import sys
    argv = list(sys.argv[1:] if argv is None else argv)
    if not any(a == "--task" or a.startswith("--task=") for a in argv):
        argv += ["--task", DEFAULT_TASK]
    return get_args(argv)


if __name__ == "__main__":
    train(_args())
