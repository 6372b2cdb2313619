"""``ScriptedPredatorGameCfg / ScriptedPredatorGameCfgPPO``: ``high_level_game`` with the reference's scripted pursuer.

Everything is ``HighLevelGameFlatCfg``'s; the one new section, ``predator``, holds the three literals of the reference's
``full_obs_predator`` (high_level_game.py:301, :307, :312)."""
from .high_level_game_flat_config import HighLevelGameFlatCfg, HighLevelGameFlatCfgPPO


class ScriptedPredatorGameCfg(HighLevelGameFlatCfg):
    class predator:
        max_lin_vel = 2.0             # speed limit per axis at the start of an episode [m/s]
        min_lin_vel = 0.01            # ... at episode step max_episode_length; linear in between and beyond (negative past ~1.005 episodes)
        gain = 2.0                    # velocity = gain x relative prey position, clamped to the limit


class ScriptedPredatorGameCfgPPO(HighLevelGameFlatCfgPPO):
    class runner(HighLevelGameFlatCfgPPO.runner):
        experiment_name = "scripted_predator_game"
