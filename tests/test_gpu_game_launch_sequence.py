"""-m gpu: WHICH launches the policy stage of the game envs issues, by name and in order, for one eager ``step_policy`` and for
``shared_actor_launch`` -- per kind of actor (feed-forward, LSTM, wide LSTM, GRU, GRU on the shared launches), with and without an opponent
pool, at wide precision 0 and with the recurrent library taken away.  The other tests check ``last_act_rc`` and bit equality between the
paths; none states the sequence, and a captured rollout graph contains exactly it.  Nothing here reads outside the tree."""
import pytest
import torch

from tests.test_gpu_dec_game import fused_pair, make_dec
from tests.test_gpu_dec_game_gru import _pair as gru_pair
from tests.test_gpu_dec_game_recurrent import _pair as lstm_pair, _recurrent_policy
from tests.test_gpu_dec_pool import member_state, prey_pool
from tests.test_gpu_dec_pool_recurrent import _rec_pool
from tests.test_gpu_game import make_game, write_ll_checkpoint
from tests.test_gpu_game_policy import high_level_actor
from tests.test_gpu_game_recurrent import _recurrent_policy as game_recurrent_policy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 64                       # two 32-env blocks: a pool's slot table names two members
# the launches of the capi layer the two envs issue, and the entry points their separate launches reach through the library objects
CAPI_LAUNCHES = ("game_pre", "game_act", "game_post", "game_lstm_act", "outcome_post", "dec_game_pre", "dec_game_act", "dec_game_post", "dec_outcome_post",
                 "dec_member_outcome_post", "dec_pool_act", "dec_lstm_step", "dec_game_lstm_act", "dec_pool_lstm_step", "dec_pool_lstm_act", "dec_gru_step",
                 "dec_game_privileged_obs")
LIBRARY_LAUNCHES = {"main": ("lg_step", "lg_policy_act", "lg_lstm_step", "lg_lstm_actor_act"), "lstm_wide": ("lg_lstm_wide_step", "lg_lstm_wide_actor_act"),
                    "gru": ("lg_gru_step",)}

DEC_REST = ("lg_step", "dec_game_post", "dec_game_privileged_obs")      # behind the policy stage of the dec env (the predator's privileged row is on)
DEC_SEPARATE = ("dec_game_pre", "lg_policy_act") + DEC_REST             # the tail of the separate launches: the clips, the low-level actor
GAME_REST = ("lg_step", "game_post")
GAME_SEPARATE = ("game_pre", "lg_policy_act") + GAME_REST
# id: (env, actors, wide precision, step_policy's launches, shared_actor_launch's launches, its answer)
TABLE = {
    "dec-ff": ("dec", "ff", 1, ("dec_game_act",) + DEC_REST, ("dec_game_act",), True),
    "dec-ff-pool": ("dec", "ff_pool", 1, ("dec_pool_act",) + DEC_REST, ("dec_game_act",), True),
    "dec-ff-precision0": ("dec", "ff", 0, ("dec_game_act", "lg_policy_act", "lg_policy_act") + DEC_SEPARATE, ("dec_game_act",), False),
    "dec-lstm": ("dec", "lstm", 1, ("dec_lstm_step", "dec_game_lstm_act") + DEC_REST, ("dec_lstm_step", "dec_game_lstm_act"), True),
    "dec-lstm-pool": ("dec", "lstm_pool", 1, ("dec_pool_lstm_step", "dec_pool_lstm_act") + DEC_REST, ("dec_pool_lstm_step", "dec_pool_lstm_act"), True),
    "dec-lstm-precision0": ("dec", "lstm", 0, ("dec_lstm_step", "lg_lstm_actor_act", "lg_lstm_actor_act") + DEC_SEPARATE, ("dec_lstm_step",), False),
    "dec-lstm-no-library": ("dec", "lstm_no_library", 1, ("lg_lstm_step", "lg_lstm_step", "lg_lstm_actor_act", "lg_lstm_actor_act") + DEC_SEPARATE, (), False),
    "dec-wide": ("dec", "wide", 1, ("lg_lstm_wide_step", "lg_lstm_wide_step", "lg_lstm_wide_actor_act", "lg_lstm_wide_actor_act") + DEC_SEPARATE, (), False),
    "dec-gru": ("dec", "gru", 1, ("lg_gru_step", "lg_gru_step", "lg_lstm_actor_act", "lg_lstm_actor_act") + DEC_SEPARATE, (), False),
    "dec-gru-shared": ("dec", "gru_shared", 1, ("dec_gru_step", "dec_game_lstm_act") + DEC_REST, ("dec_gru_step", "dec_game_lstm_act"), True),
    "game-ff": ("game", "ff", 1, ("game_act",) + GAME_REST, ("game_act",), True),
    "game-lstm": ("game", "lstm", 1, ("lg_lstm_step", "game_lstm_act") + GAME_REST, ("game_lstm_act",), True),
    "game-lstm-precision0": ("game", "lstm", 0, ("lg_lstm_step", "lg_lstm_actor_act") + GAME_SEPARATE, (), False),
    "game-gru": ("game", "gru", 1, ("lg_gru_step", "game_lstm_act") + GAME_REST, ("game_lstm_act",), True),
}


@pytest.fixture(scope="module")
def envs(tmp_path_factory):
    ckpt = write_ll_checkpoint(str(tmp_path_factory.mktemp("ll") / "model_0.pt"), seed=3)

    def predator_privileged(cfg):
        cfg.env.num_privileged_obs_predator = 10
    made = {"dec": make_dec(ckpt, N, seed=9, tweak=predator_privileged), "game": make_game(ckpt, N, seed=9)}
    for env in made.values():
        env.reset()
    return made


def _recorded(monkeypatch, names):
    """Every launch of CAPI_LAUNCHES / LIBRARY_LAUNCHES appends its name to ``names`` and runs."""
    from legged_games_gym_amd import capi

    def wrap(owner, name):
        real = getattr(owner, name)
        monkeypatch.setattr(owner, name, lambda *a, **k: names.append(name) or real(*a, **k))
    for name in CAPI_LAUNCHES:
        wrap(capi, name)
    for key, entries in LIBRARY_LAUNCHES.items():
        for name in entries:
            wrap(capi.load(key), name)


def _dec_actors(kind, env):
    """``(fused_pred, fused_prey or its pool, step_policy's keywords)`` for a row of the dec env."""
    from legged_games_gym_amd.rl.recurrent_actor import RecurrentFusedActor
    critic = dict(with_critic_memory=("prey",))
    if kind == "ff":
        return fused_pair() + ({},)
    if kind == "ff_pool":
        pred, live = fused_pair()
        pool = prey_pool(live, num_envs=N)
        assert pool.push(member_state(1)) == 1
        pool.set_slots([1, 0])
        return pred, pool, {}
    if kind in ("lstm", "lstm_no_library"):
        return lstm_pair() + (critic,)
    if kind == "lstm_pool":
        pred, live = lstm_pair()
        pool = _rec_pool(live, "prey", num_envs=N)
        assert pool.push({k: v + 0.05 for k, v in live.ac.state_dict().items()}) == 1
        pool.set_slots([1, 0])
        return pred, pool, critic
    if kind == "wide":
        pair = tuple(RecurrentFusedActor(_recurrent_policy(a, units=288), DEV, seed=s, num_envs=N, wide=True) for a, s in (("pred", 21 + 104729), ("prey", 21)))
        assert all(f.wide for f in pair)
        return pair + (critic,)
    if kind == "gru":
        return gru_pair(False) + (critic,)
    assert kind == "gru_shared"                   # the log-prob without the sample: the env keeps the sample tensor itself
    return gru_pair(True) + (dict(critic, out_pred={"log_prob": torch.empty(N, device=DEV)}, out_prey={"log_prob": torch.empty(N, device=DEV)}),)


def _game_actor(kind):
    from legged_games_gym_amd.rl import ActorCriticRecurrent, FusedActor
    from legged_games_gym_amd.rl.recurrent_actor import RecurrentFusedActor
    if kind == "ff":
        return FusedActor(high_level_actor(seed=6), DEV, seed=21)
    if kind == "lstm":
        return RecurrentFusedActor(game_recurrent_policy(), DEV, seed=21, num_envs=N)
    torch.manual_seed(6)
    ac = ActorCriticRecurrent(19, 19, 6, actor_hidden_dims=[64, 64, 32], critic_hidden_dims=[64, 64, 32], rnn_type="gru", rnn_hidden_size=64).to(DEV)
    return RecurrentFusedActor(ac, DEV, seed=21, num_envs=N, gru=True)


@pytest.mark.parametrize("row", list(TABLE))
def test_launches_of_a_policy_step_and_of_the_warm_up_call(envs, monkeypatch, row):
    from legged_games_gym_amd import capi
    which, kind, precision, want_step, want_shared, want_answer = TABLE[row]
    env = envs[which]
    if which == "dec":
        pred, prey, keywords = _dec_actors(kind, env)
        actors = (pred, prey)
    else:
        actors, keywords = (_game_actor(kind),), {}
    if kind == "lstm_no_library":                 # (the way tests/test_gpu_dec_pool_recurrent.py takes the library away)
        env._recurrent_library = lambda fused, say=True, pooled=False: (env._say_separate("forced", say, pooled), (None, False))[1]
    lib = capi.load_library()
    names = []
    old = lib.lg_mlp_wide_set_precision(precision)
    try:
        _recorded(monkeypatch, names)
        answer = env.shared_actor_launch(*actors)
        shared, names[:] = tuple(names), []
        env.step_policy(*actors, **keywords)
        stepped = tuple(names)
        torch.cuda.synchronize()
    finally:
        monkeypatch.undo()
        lib.lg_mlp_wide_set_precision(old)
        env.__dict__.pop("_recurrent_library", None)
    print(f"[observed] {row}: shared_actor_launch {answer} {shared}; step_policy {stepped}")
    assert shared == want_shared and answer is want_answer, (row, answer, shared)
    assert stepped == want_step, (row, stepped)
    if which == "dec":
        assert env.last_act_rc == (0 if want_answer else -4), row
