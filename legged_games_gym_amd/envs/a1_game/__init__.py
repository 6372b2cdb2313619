"""The predator-prey game layer (reference ``legged_gym/envs/a1_game/``): tasks ``high_level_game``, ``dec_high_level_game`` and
``scripted_predator_game``.

Importing this package registers NOTHING: the registry is a process-wide singleton and the locomotion surface is pinned to its five tasks.
``register()`` adds the game task; ``scripts/train.py`` / ``scripts/play.py`` call it when ``--task`` names one of ``TASKS``.
``register_dec()`` adds the decentralised two-policy game (``DEC_TASKS``); ``scripts/train_dec_game.py`` / ``scripts/play_dec_game.py`` call it.
``register_scripted()`` adds the prey-against-the-scripted-pursuer game (``SCRIPTED_TASKS``); ``scripts/train.py`` / ``scripts/play.py`` call it.
``set_privileged_critic(env_cfg, "prey" | "pred" | "both")`` is what ``--privileged_critic`` of the decentralised game's scripts does: it sets
``env.num_privileged_obs_prey`` / ``env.num_privileged_obs_predator`` to the widths the device writer is compiled for, before the env is made."""
from legged_games_gym_amd.utils.task_registry import task_registry

from .dec_high_level_game import DecHighLevelGame
from .dec_high_level_game_config import DecHighLevelGameCfg, DecHighLevelGameCfgPPO
from .high_level_game import HighLevelGame
from .high_level_game_flat_config import HighLevelGameFlatCfg, HighLevelGameFlatCfgPPO
from .scripted_predator_game import ScriptedPredatorGame
from .scripted_predator_game_config import ScriptedPredatorGameCfg, ScriptedPredatorGameCfgPPO

TASKS = ("high_level_game",)
DEC_TASKS = ("dec_high_level_game",)
SCRIPTED_TASKS = ("scripted_predator_game",)


def register(registry=task_registry):
    """Register ``high_level_game`` (reference ``legged_gym/envs/__init__.py``); idempotent."""
    if "high_level_game" not in registry.task_classes:
        registry.register("high_level_game", HighLevelGame, HighLevelGameFlatCfg(), HighLevelGameFlatCfgPPO())
    return registry


def unregister(registry=task_registry):
    """Take the game task out of the registry again (its three entries)."""
    for name in TASKS:
        for table in (registry.task_classes, registry.env_cfgs, registry.train_cfgs):
            table.pop(name, None)
    return registry


def register_dec(registry=task_registry):
    """Register ``dec_high_level_game`` (reference ``legged_gym/envs/__init__.py``); idempotent."""
    if "dec_high_level_game" not in registry.task_classes:
        registry.register("dec_high_level_game", DecHighLevelGame, DecHighLevelGameCfg(), DecHighLevelGameCfgPPO())
    return registry


def set_privileged_critic(env_cfg, which):
    """``--privileged_critic``: the asymmetric critic of ``dec_high_level_game`` for the prey, the predator or both (None: the config as it is)."""
    from legged_games_gym_amd import capi
    if which is None:
        return env_cfg
    if which not in ("prey", "pred", "both"):
        raise ValueError(f"--privileged_critic takes prey, pred or both, got {which!r}")
    env_cfg.env.num_privileged_obs_prey = capi.LG_DEC_NUM_PRIV_PREY if which in ("prey", "both") else None
    env_cfg.env.num_privileged_obs_predator = capi.LG_DEC_NUM_PRIV_PRED if which in ("pred", "both") else None
    return env_cfg


def unregister_dec(registry=task_registry):
    """Take the decentralised game out of the registry again (its three entries)."""
    for name in DEC_TASKS:
        for table in (registry.task_classes, registry.env_cfgs, registry.train_cfgs):
            table.pop(name, None)
    return registry


def register_scripted(registry=task_registry):
    """Register ``scripted_predator_game`` (the reference reaches it by editing high_level_game.py:188); idempotent."""
    if "scripted_predator_game" not in registry.task_classes:
        registry.register("scripted_predator_game", ScriptedPredatorGame, ScriptedPredatorGameCfg(), ScriptedPredatorGameCfgPPO())
    return registry


def unregister_scripted(registry=task_registry):
    """Take the scripted-pursuer game out of the registry again (its three entries)."""
    for name in SCRIPTED_TASKS:
        for table in (registry.task_classes, registry.env_cfgs, registry.train_cfgs):
            table.pop(name, None)
    return registry
