"""The structure ``rl/runner.py`` promises: every attribute the runner reads on itself is declared before a rollout runs (no lazy
``getattr(self, "_x", None)``), and the capture rollback is the envs' -- an agent view has no setters left for the runner to reach through."""
import os
import re

from legged_games_gym_amd.rl import OnPolicyRunner

SOURCE = open(os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(__file__))), "legged_games_gym_amd", "rl", "runner.py")).read()


def test_agent_view_has_no_setters_for_the_capture_rollback():
    from legged_games_gym_amd.envs.a1_game.dec_high_level_game import AgentView
    for name in ("_obs_flip", "obs_buf", "_capturing"):
        prop = vars(AgentView).get(name)
        assert prop is None or (isinstance(prop, property) and prop.fset is None), name
    assert "_obs_pair" not in vars(AgentView)
    assert AgentView.common_step_counter.fset is not None          # (learn advances the counter after a replay)


def test_game_base_has_no_capturing_setter_and_the_envs_have_the_pair():
    from legged_games_gym_amd.envs import LeggedRobot
    from legged_games_gym_amd.envs.a1_game.dec_high_level_game import AgentView, DecHighLevelGame
    from legged_games_gym_amd.envs.a1_game.game_base import GameBase
    from legged_games_gym_amd.envs.a1_game.high_level_game import HighLevelGame
    assert GameBase._capturing.fset is None and GameBase.common_step_counter.fset is not None
    for cls in (LeggedRobot, GameBase, HighLevelGame, DecHighLevelGame, AgentView):
        assert callable(getattr(cls, "capture_state")) and callable(getattr(cls, "abort_graph_capture")), cls.__name__


def test_every_private_name_the_runner_reads_on_itself_is_declared_on_a_bare_runner():
    r = OnPolicyRunner.__new__(OnPolicyRunner)
    r._init_rollout_state()
    names = sorted(set(re.findall(r"\bself\.(_[A-Za-z0-9_]+)", SOURCE)))
    assert {"_fused", "_game_rollout", "_recurrent_rollout", "_rolled", "_time_outs", "_priv_carry", "_critic_fwd", "_roll"} <= set(names)
    missing = [n for n in names if not hasattr(r, n)]
    assert not missing, missing
    # the "not yet" values: the generic loop, nothing decided, nothing allocated
    assert r._fused is None and r._game_rollout is False and r._recurrent_rollout is False
    for name in ("_fused_step", "_rolled", "_roll", "_time_outs", "_critic_features", "_priv_carry", "_critic_fwd", "_critic_chunks", "_critic_out"):
        assert getattr(r, name) is None, name
    declared = sorted(vars(r))
    r.use_generic_loop()
    assert sorted(vars(r)) == declared and r._fused is None


def test_no_lazy_getattr_on_self_remains_in_the_runner():
    lazy = re.findall(r'getattr\(self, "(\w+)"', SOURCE)
    assert lazy == ["alg"], lazy


def test_the_runner_does_not_name_what_the_envs_roll_back():
    for word in ("_obs_flip", "_obs_pair", "set_obs_output", "set_deferred_extras", "_capturing"):
        assert word not in SOURCE, word
    body = SOURCE[SOURCE.index("def _try_build_graphed_rollout"):SOURCE.index("def _new_stats")]
    assert "ll_env" not in body and "capture_state()" in body and "abort_graph_capture(snapshot)" in body


def test_there_is_one_device_rollout_loop_and_one_place_that_makes_a_device_actor():
    assert SOURCE.count("lg_rollout_record(") == 1 and SOURCE.count("def _rollout_steps_device") == 1
    assert "_rollout_steps_fused" not in SOURCE and "_rollout_steps_game" not in SOURCE
    assert len(re.findall(r"import RecurrentFusedActor\b", SOURCE)) == 1 and len(re.findall(r"import FusedActor\b", SOURCE)) == 1
    assert SOURCE.count("except Exception as exc") == 2              # the actor builder's and the graph capture's


def test_new_stats_takes_the_callers_running_sums():
    import torch
    r = OnPolicyRunner.__new__(OnPolicyRunner)
    r.env, r.device = type("E", (), {"num_envs": 5})(), "cpu"
    s = r._new_stats()
    assert sorted(s) == ["_sums", "count", "cur_len", "cur_rew", "sum_len", "sum_rew"] and s["cur_rew"].shape == (5,) and s["_sums"].shape == (3,)
    s["_sums"].copy_(torch.tensor([1.0, 2.0, 3.0]))
    assert (float(s["sum_rew"]), float(s["sum_len"]), float(s["count"])) == (1.0, 2.0, 3.0)      # views of the one buffer
    mine = torch.ones(5), torch.ones(5)
    s = r._new_stats(*mine)
    assert s["cur_rew"] is mine[0] and s["cur_len"] is mine[1]
