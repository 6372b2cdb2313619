"""Host-side helpers with the reference's names and semantics.

Mirrors the in-scope part of reference ``legged_gym/utils/helpers.py``:
``class_to_dict`` (:41-56, defines the *alphabetical* reward order through
``dir()``), ``update_class_from_dict`` (:58-65), ``set_seed`` (:67-77),
``parse_sim_params`` (:79-101), ``get_load_path`` (:103-125),
``update_cfg_from_args`` (:159-182) and ``get_args`` (:184-210).  The Isaac Gym
``gymutil.parse_arguments`` call is replaced by ``argparse`` exposing the same
flag names; ``export_policy_as_jit`` (:212-222, feed-forward actors); the recurrent exporter and the game-layer
loaders are out of scope.
"""
import argparse
import os
import random

import numpy as np
import torch


def class_to_dict(obj):
    """Config object -> plain dict, keys in ``dir()`` (alphabetical) order."""
    if not hasattr(obj, "__dict__"):
        return obj
    out = {}
    for key in dir(obj):
        if key.startswith("_"):
            continue
        val = getattr(obj, key)
        if isinstance(val, list):
            out[key] = [class_to_dict(v) for v in val]
        else:
            out[key] = class_to_dict(val)
    return out


def update_class_from_dict(obj, dct):
    for key, val in dct.items():
        attr = getattr(obj, key, None)
        if isinstance(attr, type):
            update_class_from_dict(attr, val)
        else:
            setattr(obj, key, val)


def set_seed(seed):
    """Seeds python, numpy and torch (CPU + all GPUs); -1 draws a seed."""
    if seed == -1:
        seed = np.random.randint(0, 10000)
    print("Setting seed: {}".format(seed))
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    os.environ["PYTHONHASHSEED"] = str(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(seed)
        torch.cuda.manual_seed_all(seed)
    return seed


class SimParams:
    """Plain-attribute stand-in for ``gymapi.SimParams`` (external type).

    Holds exactly the fields the env reads: ``dt``, ``substeps``, ``gravity``,
    ``up_axis``, ``use_gpu_pipeline`` and a ``physx`` namespace.
    """

    class _NS:
        pass

    def __init__(self):
        self.dt = 1.0 / 60.0
        self.substeps = 2
        self.gravity = [0.0, 0.0, -9.81]
        self.up_axis = 1
        self.use_gpu_pipeline = True
        self.physx = SimParams._NS()
        self.physx.use_gpu = True
        self.physx.num_subscenes = 0
        self.physx.num_threads = 0

    def __repr__(self):
        return f"SimParams(dt={self.dt}, substeps={self.substeps}, gravity={self.gravity})"


def parse_sim_params(args, cfg):
    """``{"sim": {...}}`` dict -> SimParams, command-line overrides applied."""
    sp = SimParams()
    sp.physx.use_gpu = getattr(args, "use_gpu", True)
    sp.physx.num_subscenes = getattr(args, "subscenes", 0)
    sp.use_gpu_pipeline = getattr(args, "use_gpu_pipeline", True)
    sim = cfg.get("sim", {}) if isinstance(cfg, dict) else {}
    for key, val in sim.items():
        if key == "physx":
            for k2, v2 in val.items():
                setattr(sp.physx, k2, v2)
        else:
            setattr(sp, key, val)
    if getattr(args, "num_threads", 0) and args.num_threads > 0:
        sp.physx.num_threads = args.num_threads
    return sp


def get_load_path(root, load_run=-1, checkpoint=-1):
    """Latest run dir (lexicographic) and highest ``model_*.pt`` (zero-padded key)."""
    try:
        runs = sorted(os.listdir(root))
        if "exported" in runs:
            runs.remove("exported")
        last_run = os.path.join(root, runs[-1])
    except Exception:
        raise ValueError("No runs in this directory: " + root)
    load_run = last_run if load_run == -1 else os.path.join(root, load_run)
    if checkpoint == -1:
        models = [f for f in os.listdir(load_run) if "model" in f]
        models.sort(key=lambda m: "{0:0>15}".format(m))
        model = models[-1]
    else:
        model = "model_{}.pt".format(checkpoint)
    return os.path.join(load_run, model)


def update_cfg_from_args(env_cfg, cfg_train, args):
    if env_cfg is not None and args.num_envs is not None:
        env_cfg.env.num_envs = args.num_envs
    if cfg_train is not None:
        if args.seed is not None:
            cfg_train.seed = args.seed
        if args.max_iterations is not None:
            cfg_train.runner.max_iterations = args.max_iterations
        if getattr(args, "max_evolutions", None) is not None:
            cfg_train.runner.max_evolutions = args.max_evolutions
        if args.resume:
            cfg_train.runner.resume = args.resume
        for name in ("experiment_name", "run_name", "load_run", "checkpoint"):
            val = getattr(args, name)
            if val is not None:
                setattr(cfg_train.runner, name, val)
    return env_cfg, cfg_train


class _LstmPolicy(torch.nn.Module):
    """Deployment copy of a recurrent policy for one robot: the actor behind its LSTM, the hidden and cell state kept in a buffer
    between calls of ``forward(x)``; ``reset_memory()`` zeroes them (what the reference's exporter writes for an LSTM policy)."""

    def __init__(self, actor, rnn):
        super().__init__()
        self.actor, self.memory = actor, rnn
        # one stacked buffer for both halves of the state: state[0] = h, state[1] = c, each [layers, 1, H]
        self.register_buffer("state", torch.zeros(2, rnn.num_layers, 1, rnn.hidden_size))

    def forward(self, x):
        seq = x.view(1, 1, -1)                                   # one robot, one step
        features, (h, c) = self.memory(seq, (self.state[0], self.state[1]))
        self.state.copy_(torch.stack([h, c]))
        return self.actor(features.view(1, -1))

    @torch.jit.export
    def reset_memory(self):
        self.state.zero_()


def export_policy_as_jit(actor_critic, path):
    """TorchScript copy of the policy for deployment (reference helpers.py:212-222): ``<path>/policy_1.pt`` holds the actor of a
    feed-forward policy; for an LSTM policy ``<path>/policy_lstm_1.pt`` holds memory + actor with the state in buffers."""
    import copy
    os.makedirs(path, exist_ok=True)
    if hasattr(actor_critic, "memory_a"):
        rnn = actor_critic.memory_a.rnn
        if not isinstance(rnn, torch.nn.LSTM):
            raise NotImplementedError(f"recurrent policy export covers the LSTM only, not {type(rnn).__name__}")
        target = os.path.join(path, "policy_lstm_1.pt")
        module = _LstmPolicy(copy.deepcopy(actor_critic.actor), copy.deepcopy(rnn)).to("cpu").eval()
        torch.jit.script(module).save(target)
        return target
    target = os.path.join(path, "policy_1.pt")
    actor = copy.deepcopy(actor_critic.actor).to("cpu").eval()
    torch.jit.script(actor).save(target)
    return target


def apply_policy_args(train_cfg, args):
    """``--policy_class_name`` / ``--rnn_*`` onto a train cfg: a runner key and policy keyword arguments of ``ActorCriticRecurrent``,
    set on the instance so that the config classes keep the reference's fields."""
    if getattr(args, "policy_class_name", None) is not None:
        train_cfg.runner.policy_class_name = args.policy_class_name
    for name in ("rnn_type", "rnn_hidden_size", "rnn_num_layers"):
        if getattr(args, name, None) is not None:
            setattr(train_cfg.policy, name, getattr(args, name))
    return train_cfg


def get_args(argv=None):
    """Same flags as the reference CLI (helpers.py:185-203 + the gymutil set)."""
    p = argparse.ArgumentParser(description="RL Policy")
    p.add_argument("--task", type=str, default="anymal_c_flat")
    p.add_argument("--resume", action="store_true", default=False)
    p.add_argument("--experiment_name", type=str)
    p.add_argument("--run_name", type=str)
    p.add_argument("--load_run", type=str)
    p.add_argument("--checkpoint", type=int)
    p.add_argument("--headless", action="store_true", default=False)
    p.add_argument("--horovod", action="store_true", default=False)   # dead flag in the reference too
    p.add_argument("--rl_device", type=str, default="cuda:0")
    p.add_argument("--num_envs", type=int)
    p.add_argument("--seed", type=int)
    p.add_argument("--max_iterations", type=int)
    p.add_argument("--device_rollout", action="store_true", default=False,
                   help="high_level_game: train on the device rollout (runner key of the same name: MFMA high-level actor, three launches per step, one graph "
                        "replay per rollout); an actor shape the kernels refuse falls back to the generic loop with a message")
    p.add_argument("--device_bptt", action="store_true", default=False,
                   help="ActorCriticRecurrent on the GPU: run the LSTM recurrence of the PPO update, forward and backward through time, on the device sequence "
                        "kernels (runner key of the same name); a memory they do not cover (GRU, several layers, more than 256 units) keeps torch with a message")
    p.add_argument("--wide_memory", action="store_true", default=False,
                   help="ActorCriticRecurrent on the GPU: run LSTM memories of 288 .. 512 units on the device rollout (runner key of the same name: the cell "
                        "and actor kernels of liblegged_lstm_wide.so; the game tasks then issue separate launches); off, such a memory falls back or is refused")
    p.add_argument("--device_gru", action="store_true", default=False,
                   help="ActorCriticRecurrent with --rnn_type gru on the GPU: run the GRU memories (one layer, up to 256 units) on the device rollout (runner key "
                        "of the same name: the cell kernel of liblegged_gru.so; dec_high_level_game then issues separate launches unless --dec_gru_shared is given "
                        "as well); off, a GRU falls back or is refused")
    p.add_argument("--dec_gru_shared", action="store_true", default=False,
                   help="dec_high_level_game with --rnn_type gru --device_gru: advance the GRU memories of both agents in one launch (runner key of the same "
                        "name: lg_dec_gru_step of liblegged_dec_game_gru.so) and run the three actors in lg_dec_game_lstm_act, two launches per policy step "
                        "where --device_gru alone takes six (a training rollout adds torch's log-prob of the learner's sample, so that it stores what it stores "
                        "without the flag, bit for bit); without --device_gru or with an LSTM the runner refuses it")
    p.add_argument("--outcome_stats", action="store_true", default=False,
                   help="the game tasks (dec_high_level_game: scripts/train_dec_game.py): count inside the post-step launch why episodes end (captured, left the arena, fell, "
                        "survived) and log the rates as Episode/outcome_*; the scripts set env.outcome_stats on the registration they use")
    p.add_argument("--policy_class_name", type=str, help="ActorCritic or ActorCriticRecurrent (runner key of the same name)")
    p.add_argument("--rnn_type", type=str, help="ActorCriticRecurrent: lstm or gru")
    p.add_argument("--rnn_hidden_size", type=int, help="ActorCriticRecurrent: units of each memory (the device rollout covers multiples of 32 up to 256, with --wide_memory up to 512)")
    p.add_argument("--rnn_num_layers", type=int, help="ActorCriticRecurrent: layers of each memory (the device rollout covers 1)")
    p.add_argument("--max_evolutions", type=int, help="dec_high_level_game: how often predator and prey alternate (scripts/train_dec_game.py)")
    p.add_argument("--opponent_pool", type=int, default=0,
                   help="dec_high_level_game with --device_rollout: train each agent against a pool of this many frozen earlier versions of its opponent "
                        "besides the live one (runner key opponent_pool_size; 0 = off, at most 15)")
    p.add_argument("--opponent_latest_share", type=float, default=0.5,
                   help="with --opponent_pool: the share of the 32-env blocks that meet the live opponent (runner key opponent_latest_share)")
    p.add_argument("--opponent_priority", type=float, default=0.0,
                   help="with --opponent_pool and --outcome_stats: deal the non-live blocks in proportion to (1 - learner's win rate against the member) ** P "
                        "instead of round-robin (runner key opponent_priority; 0 = off)")
    p.add_argument("--opponent_pool_recurrent", action="store_true", default=False,
                   help="with --opponent_pool and --policy_class_name ActorCriticRecurrent: the pools hold recurrent snapshots (runner key "
                        "opponent_pool_recurrent; the actor memory and the actor MLP of a 32-env block are its pool member's)")
    p.add_argument("--privileged_critic", type=str, default=None, choices=("prey", "pred", "both"),
                   help="dec_high_level_game (scripts/train_dec_game.py, play_dec_game.py, crossplay_dec_game.py): an asymmetric critic for that agent -- it reads "
                        "the simulator's true state (env.num_privileged_obs_prey = 22 / env.num_privileged_obs_predator = 10), the actor keeps the sensor's view; "
                        "the play scripts need it to rebuild a critic of the checkpoint's shape")
    # flags gymutil.parse_arguments contributes
    p.add_argument("--sim_device", type=str, default="cuda:0")
    p.add_argument("--pipeline", type=str, default="gpu")
    p.add_argument("--graphics_device_id", type=int, default=0)
    p.add_argument("--num_threads", type=int, default=0)
    p.add_argument("--subscenes", type=int, default=0)
    p.add_argument("--physx", action="store_true", default=True)
    args = p.parse_args(argv)
    dev = args.sim_device
    args.sim_device_type = dev.split(":")[0]
    args.compute_device_id = int(dev.split(":")[1]) if ":" in dev else 0
    args.sim_device_id = args.compute_device_id
    args.use_gpu = args.sim_device_type == "cuda"
    args.use_gpu_pipeline = args.use_gpu and args.pipeline.lower() in ("gpu", "cuda")
    args.physics_engine = "physx"
    args.device = args.sim_device_type
    return args
