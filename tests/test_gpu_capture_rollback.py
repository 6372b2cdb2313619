"""The rollback of a rollout-graph capture that failed is the envs': ``capture_state()`` / ``abort_graph_capture(state)`` on ``LeggedRobot``,
the game envs and an agent view of ``dec_high_level_game``, and the runner's fall-back to eager steps on top of them.  Host logic: the
smallest sizes that build the tasks (64 envs)."""
import pytest
import torch

from tests.game_fixtures import game_registered  # noqa: F401
from tests.test_gpu_dec_game import make_dec
from tests.test_gpu_game import make_game, write_ll_checkpoint
from tests.test_gpu_game_policy import game_runner

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 64
NAN = float("nan")
STORED = ("observations", "actions", "mu", "sigma", "actions_log_prob", "rewards", "dones", "values")


def _anymal(**runner_keys):
    """A 64-env ``anymal_c_flat`` env and, given runner keys or not, its runner (the same initial policy on every call)."""
    from legged_games_gym_amd.envs import task_registry
    from legged_games_gym_amd.utils import get_args
    args = get_args(["--task", "anymal_c_flat", "--num_envs", str(N), "--headless", "--sim_device", DEV, "--rl_device", DEV])
    env, _ = task_registry.make_env("anymal_c_flat", args)
    _, train_cfg = task_registry.get_cfgs("anymal_c_flat")
    for key, value in runner_keys.items():
        setattr(train_cfg.runner, key, value)
    try:
        torch.manual_seed(1234)
        runner, _ = task_registry.make_alg_runner(env, "anymal_c_flat", args, train_cfg=train_cfg, log_root=None)
    finally:
        for key in runner_keys:
            delattr(train_cfg.runner, key)
    return env, runner


class Pair:
    """One observation pair of an env in the NaN stage.  The step that follows writes ``pair[flip ^ 1]``: that buffer is filled with NaN.
    The other one is too where the step does not read it; a buffer the step reads -- the game observations carry three past sensed positions
    over (``GameHistory``), the low-level policy acts on the low-level env's current observations -- keeps its contents, and "not written"
    is then that they are bit for bit what they were, instead of still all NaN."""

    def __init__(self, name, pair, flip, read_by_the_step):
        self.name, self.new, self.old = name, pair[flip ^ 1], pair[flip]
        self.new.fill_(NAN)
        self.kept = self.old.clone() if read_by_the_step else None
        if not read_by_the_step:
            self.old.fill_(NAN)

    def check(self):
        assert bool(torch.isfinite(self.new).all()), self.name
        assert bool(torch.isnan(self.old).all()) if self.kept is None else torch.equal(self.old, self.kept), self.name


def _cases(tmp_path, task, through):
    """``(env the two methods are called on, step(), current buffers -> pair members expected, pairs of the NaN stage)``."""
    zeros = lambda n: torch.zeros(N, n, device=DEV)
    if task == "anymal_c_flat":
        env, _ = _anymal()
        env.reset()
        current = lambda: [(env.obs_buf, env._obs_pair)]
        pairs = lambda f: [Pair("obs", env._obs_pair, f["own"], False)]
        return env, env, lambda: env.step(zeros(env.num_actions))[0], current, pairs
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    if task == "high_level_game":
        env = make_game(ckpt, N, seed=9)
        torch.manual_seed(90)
        env.reset()
        current = lambda: [(env.obs_buf, env._obs_pair), (env.ll_env.obs_buf, env.ll_env._obs_pair)]
        pairs = lambda f: [Pair("obs", env._obs_pair, f["own"], True), Pair("low-level obs", env.ll_env._obs_pair, f["ll"], True)]
        return env, env, lambda: env.step(zeros(6))[0], current, pairs

    def prey_on(cfg):
        cfg.env.num_privileged_obs_prey = 22
    env = make_dec(ckpt, N, seed=9, tweak=prey_on)
    torch.manual_seed(90)
    env.reset()
    view = env.agent_view("prey", lambda obs: zeros(2))
    current = lambda: [(env.obs_buf_prey, env._obs_pair_prey), (env.obs_buf_pred, env._obs_pair_pred), (env.privileged_obs_buf_prey, env._priv_pair["prey"]),
                       (view.obs_buf, env._obs_pair_prey), (view.get_privileged_observations(), env._priv_pair["prey"]),
                       (env.ll_env.obs_buf, env.ll_env._obs_pair)]
    pairs = lambda f: [Pair("prey obs", env._obs_pair_prey, f["own"], True), Pair("pred obs", env._obs_pair_pred, f["own"], False),
                       Pair("privileged prey", env._priv_pair["prey"], f["own"], False), Pair("low-level obs", env.ll_env._obs_pair, f["ll"], True)]
    if through == "view":
        return env, view, lambda: view.step(zeros(4))[0], current, pairs
    return env, env, lambda: env.step(zeros(2), zeros(4))[1], current, pairs


@pytest.mark.parametrize("task,through", [("anymal_c_flat", "env"), ("high_level_game", "env"), ("dec_high_level_game", "env"), ("dec_high_level_game", "view")])
def test_abort_puts_the_flips_the_buffers_the_binding_and_the_counter_back(tmp_path, task, through):
    """No capture involved: an odd number of eager steps leaves every flip on the other side, ``abort_graph_capture`` puts the env back on
    the snapshot's, and the next step writes the other buffer of every pair -- the sim's output binding came back with the flip."""
    env, target, step, current, pairs = _cases(tmp_path, task, through)
    ll = getattr(env, "ll_env", env)
    snap = target.capture_state()
    flips = {"own": env._obs_flip, "ll": ll._obs_flip}
    counter = target.common_step_counter
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    assert target.capture_state() != snap and env._obs_flip != flips["own"] and ll._obs_flip != flips["ll"]
    target.abort_graph_capture(snap)
    assert target.capture_state() == snap
    assert env._obs_flip == flips["own"] and ll._obs_flip == flips["ll"]
    for k, (buf, pair) in enumerate(current()):
        assert buf is pair[flips["ll"] if pair is ll._obs_pair and ll is not env else flips["own"]], k
    assert target.common_step_counter == counter and ll.common_step_counter == counter
    assert target._capturing is False and ll._capturing is False
    stage = pairs(flips)
    obs = step()
    torch.cuda.synchronize()
    assert obs is current()[0 if through == "env" else 3][0] and bool(torch.isfinite(obs).all())
    assert any(obs is p.new for p in stage)
    for p in stage:
        p.check()
    assert target.common_step_counter == counter + 1


def _refuse_capture(env, monkeypatch):
    def refuse():
        raise RuntimeError("refused")                  # a host exception before any stream capture starts
    monkeypatch.setattr(env, "begin_graph_capture", refuse)


def _check_fallback_equals_eager(env_a, run_a, env_b, run_b, monkeypatch, capsys):
    assert run_a._fused is not None and run_b._fused is not None
    assert run_b._try_build_graphed_rollout() is None                      # graphed_rollout = False: not a word, nothing run
    assert env_a.capture_state() == env_b.capture_state()
    _refuse_capture(env_a, monkeypatch)
    capsys.readouterr()
    assert run_a._try_build_graphed_rollout() is None
    out = capsys.readouterr().out
    assert "[runner] graphed rollout unavailable (RuntimeError: refused); using eager steps" in out, out
    assert run_a.alg.storage.step == 0
    with torch.inference_mode():
        run_a._rollout_steps(run_a._new_stats())                           # the warm-up rollout plus one ...
        stats = run_b._new_stats()
        run_b._rollout_steps(stats)                                        # ... and the same two as plain rollouts
        run_b.alg.storage.clear()
        run_b._rollout_steps(stats)
    torch.cuda.synchronize()
    sa, sb = run_a.alg.storage, run_b.alg.storage
    for name in STORED:
        assert torch.equal(getattr(sa, name), getattr(sb, name)), name
    assert bool(torch.isfinite(sa.values).all()) and float(sa.values.abs().max()) > 0
    assert env_a.capture_state() == env_b.capture_state() and env_a._capturing is False
    assert torch.equal(env_a.get_observations(), env_b.get_observations())


def test_runner_falls_back_to_eager_steps_on_anymal_c_flat(monkeypatch, capsys):
    env_a, run_a = _anymal()
    env_b, run_b = _anymal(graphed_rollout=False)
    _check_fallback_equals_eager(env_a, run_a, env_b, run_b, monkeypatch, capsys)


def test_runner_falls_back_to_eager_steps_on_high_level_game(tmp_path, monkeypatch, capsys, game_registered):
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    env_a, run_a = game_runner(game_registered, tmp_path, monkeypatch, ckpt, N)
    env_b, run_b = game_runner(game_registered, tmp_path, monkeypatch, ckpt, N, graphed_rollout=False)
    assert run_a._game_rollout and run_b._game_rollout
    _check_fallback_equals_eager(env_a, run_a, env_b, run_b, monkeypatch, capsys)
