"""``ScriptedPredatorGame`` -- ``high_level_game`` with the prey alone learning, against the reference's scripted pursuer.

The predator sees the prey at all times, heads straight for it and "loses steam" as the episode runs out (reference
``full_obs_predator('integrator')``, high_level_game.py:289-324, which ``step_predator_single_integrator(command=None)`` calls).  In the
reference this is an edit of line 188; here it is a task.  Every step path of ``HighLevelGame`` -- ``step``, the graphed step,
``step_policy`` (three launches: ``lg_game_act`` -> ``lg_step`` -> ``lg_pursuer_post``), the graphed policy step and the runner's captured
device rollout -- issues ``lg_pursuer_post`` (include/legged_pursuer_game.h) where the parent issues ``lg_game_post``.

The policy stays the reference's 19 -> 6 one: columns 4:6 of the command are clipped and stored, and then ignored (DESIGN.md section 8,
G16).  ``predator_command`` [num_envs, 2] holds the velocity the kernel integrated in the last step."""
import torch

from legged_games_gym_amd import capi

from .high_level_game import HighLevelGame


def check_predator_cfg(cfg):
    """The ``predator`` section of the config, or a ValueError that names the offending field."""
    c = cfg.predator
    for name in ("max_lin_vel", "min_lin_vel", "gain"):
        v = getattr(c, name)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v:
            raise ValueError(f"predator.{name} must be a number, got {v!r}")
    if c.max_lin_vel < c.min_lin_vel:
        raise ValueError(f"predator.max_lin_vel ({c.max_lin_vel}) must not be below predator.min_lin_vel ({c.min_lin_vel})")
    if not c.gain > 0:
        raise ValueError(f"predator.gain must be positive, got {c.gain}")
    return c


class ScriptedPredatorGame(HighLevelGame):
    TASK = "scripted_predator_game"

    def __init__(self, cfg, sim_params, physics_engine, sim_device, headless):
        check_predator_cfg(cfg)                     # refuse a bad rule before the low-level env and its checkpoint are built
        super().__init__(cfg, sim_params, physics_engine, sim_device, headless)

    def _init_buffers(self):
        super()._init_buffers()
        self.predator_command = torch.zeros(self.num_envs, 2, device=self.device, dtype=torch.float)

    def _pack(self):
        super()._pack()
        c = check_predator_cfg(self.cfg)
        Q = capi.lg_pursuer_params()
        Q.max_lin_vel, Q.min_lin_vel, Q.gain = float(c.max_lin_vel), float(c.min_lin_vel), float(c.gain)
        Q.max_episode_length = int(self.max_episode_length)
        self._Q = Q

    def _post(self, B, common_step_counter, stream):
        if self._outcome is None:
            capi.pursuer_post(self._P, self._Q, B, self.predator_command.data_ptr(), common_step_counter, stream)
        else:                                       # outcome statistics on (HighLevelGame.enable_outcome_stats): same outputs, plus the counts
            capi.outcome_pursuer_post(self._P, self._Q, B, self._outcome, self.predator_command.data_ptr(), common_step_counter, stream)
