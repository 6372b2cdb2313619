"""Task registration (reference ``legged_gym/envs/__init__.py:32-56``): the five locomotion tasks.

The predator-prey task ``high_level_game`` (``envs/a1_game``) is NOT registered by this import: the registry is a process-wide singleton
whose locomotion surface is pinned, so ``legged_games_gym_amd.envs.a1_game.register()`` adds it on demand (``scripts/train.py`` and
``scripts/play.py`` call it when ``--task`` names it).  ``dec_high_level_game`` (``register_dec()``, ``scripts/train_dec_game.py``) and
``scripted_predator_game`` (``register_scripted()``) are built and registered on demand in the same way; ``low_level_game`` as a task of
its own is not built.

``dec_high_level_game`` can give either agent an asymmetric critic: with ``env.num_privileged_obs_prey = 22`` and / or
``env.num_privileged_obs_predator = 10`` (``--privileged_critic {prey,pred,both}`` of its scripts) the env writes privileged observations for
that agent's critic -- the true relative position, the prey's heading, the episode clock -- with one more launch per step, and the runners
size the critic from them; the actor keeps the sensor's view.  The two single-policy game tasks have no privileged observations (their
policy already reads the true relative position) and say so.
"""
from .base.legged_robot import LeggedRobot
from .anymal_c.anymal import Anymal
from .cassie.cassie import Cassie
from .configs import (LeggedRobotCfg, LeggedRobotCfgPPO, AnymalCRoughCfg, AnymalCRoughCfgPPO, AnymalCFlatCfg,
                      AnymalCFlatCfgPPO, AnymalBRoughCfg, AnymalBRoughCfgPPO, A1RoughCfg, A1RoughCfgPPO,
                      CassieRoughCfg, CassieRoughCfgPPO)
from legged_games_gym_amd.utils.task_registry import task_registry

task_registry.register("anymal_c_rough", Anymal, AnymalCRoughCfg(), AnymalCRoughCfgPPO())
task_registry.register("anymal_c_flat", Anymal, AnymalCFlatCfg(), AnymalCFlatCfgPPO())
task_registry.register("anymal_b", Anymal, AnymalBRoughCfg(), AnymalBRoughCfgPPO())
task_registry.register("a1", LeggedRobot, A1RoughCfg(), A1RoughCfgPPO())
task_registry.register("cassie", Cassie, CassieRoughCfg(), CassieRoughCfgPPO())
