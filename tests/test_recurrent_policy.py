"""The recurrent policy without a GPU: ``ActorCriticRecurrent`` / ``Memory`` (rsl_rl's names), the rollout mode against a float64
restatement, the once-per-rollout state storage and ``recurrent_mini_batch_generator`` pinned by replaying two consecutive rollouts in
batch mode, ``PPO.update`` through time, the runner, the exporter and the command-line flags."""
import os

import numpy as np
import pytest
import torch

from legged_games_gym_amd.rl import PPO, ActorCriticRecurrent, OnPolicyRunner
from legged_games_gym_amd.rl.actor_critic import split_and_pad_trajectories, unpad_trajectories
from tests import recurrent_ref
from tests.recurrent_ref import actor_forward64, actor_params64, lstm_params64, lstm_step64, saturating_bias

KEYS = (["std"] + [f"{net}.{i}.{w}" for net in ("actor", "critic") for i in (0, 2, 4, 6) for w in ("weight", "bias")]
        + [f"memory_{m}.rnn.{w}" for m in ("a", "c") for w in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")])


def _policy(I=5, Ic=5, A=3, H=8, **kw):
    torch.manual_seed(0)
    return ActorCriticRecurrent(I, Ic, A, actor_hidden_dims=[16, 16, 16], critic_hidden_dims=[16, 16, 16], rnn_hidden_size=H, **kw)


class StubEnv:
    """A VecEnv with scripted dones: observations are a fixed random sequence, ``dones[t]`` comes from ``pattern[t % len(pattern)]``."""

    def __init__(self, N, I, A, pattern, seed=0):
        self.num_envs, self.num_obs, self.num_privileged_obs, self.num_actions = N, I, None, A
        self.max_episode_length, self.device = 100, "cpu"
        self.pattern = torch.as_tensor(pattern, dtype=torch.bool)
        self.gen = torch.Generator().manual_seed(seed)
        self.t = 0
        self.episode_length_buf = torch.zeros(N, dtype=torch.long)
        self.obs = self._draw()
        self.extras = {}

    def _draw(self):
        return torch.rand(self.num_envs, self.num_obs, generator=self.gen) * 6.0 - 3.0

    def get_observations(self):
        return self.obs

    def get_privileged_observations(self):
        return None

    def reset(self):
        return self.obs, None

    def step(self, actions):
        dones = self.pattern[self.t % len(self.pattern)].clone()
        self.t += 1
        self.obs = self._draw()
        rew = torch.rand(self.num_envs, generator=self.gen)
        return self.obs, None, rew, dones, {"time_outs": torch.zeros(self.num_envs, dtype=torch.bool)}


def test_state_dict_keys_and_gru():
    ac = _policy()
    assert list(ac.state_dict().keys()) == KEYS and ac.is_recurrent is True
    assert ac.get_hidden_states() == (None, None)
    ac.reset(torch.zeros(4, dtype=torch.bool))               # nothing carried yet: a no-op, as for the feed-forward class
    gru = _policy(rnn_type="gru")
    assert isinstance(gru.memory_a.rnn, torch.nn.GRU)
    with torch.no_grad():
        a = gru.act(torch.randn(4, 5))
        v = gru.evaluate(torch.randn(4, 5))
    assert a.shape == (4, 3) and v.shape == (4, 1) and gru.memory_a.hidden_states.shape == (1, 4, 8)
    gru.reset(torch.tensor([True, False, False, True]))
    assert float(gru.memory_a.hidden_states[0, 0].abs().sum()) == 0.0 and float(gru.memory_a.hidden_states[0, 1].abs().sum()) > 0.0
    with pytest.raises(ValueError):
        _policy(rnn_type="rnn")


def test_rollout_mode_matches_float64_restatement():
    I, H, N, T = 5, 8, 7, 12
    ac = _policy(I=I, Ic=I, H=H)
    gen = torch.Generator().manual_seed(1)
    xs = torch.rand(T, N, I, generator=gen) * 6.0 - 3.0
    dones = torch.zeros(T, N, dtype=torch.bool)
    dones[0, 0] = True                                       # done at t = 0
    dones[4, 1] = dones[5, 1] = True                         # done twice in a row
    dones[7, 3] = dones[10, 5] = True                        # (env 2 is never done)
    pa, pc = lstm_params64(ac.memory_a.rnn), lstm_params64(ac.memory_c.rnn)
    actor64 = lambda h: _mlp64(ac.actor, h)
    critic64 = lambda h: _mlp64(ac.critic, h)
    ha = ca = hc = cc = np.zeros((N, H))
    with torch.no_grad():
        for t in range(T):
            reset = dones[t - 1].numpy() if t else None
            ha, ca = lstm_step64(pa, xs[t].numpy(), ha, ca, reset)
            hc, cc = lstm_step64(pc, xs[t].numpy(), hc, cc, reset)
            mean = ac.act_inference(xs[t])
            val = ac.evaluate(xs[t])
            ac.reset(dones[t])
            assert np.abs(mean.double().numpy() - actor64(ha)).max() < 1e-5, t
            assert np.abs(val.double().numpy() - critic64(hc)).max() < 1e-5, t
    (h_a, c_a), (h_c, c_c) = ac.get_hidden_states()
    keep = (~dones[T - 1]).double().numpy()[:, None]
    assert np.abs(h_a[0].double().numpy() - ha * keep).max() < 1e-5 and np.abs(c_c[0].double().numpy() - cc * keep).max() < 1e-5


def _lstm_case(saturate, I=19, H=64, N=5, T=6):
    """A default-initialised ``nn.LSTM`` (optionally with the saturating biases), ``x`` uniform in [-3, 3] and reset flags on some rows."""
    torch.manual_seed(4)
    rnn = torch.nn.LSTM(I, H)
    if saturate:
        with torch.no_grad():
            rnn.bias_ih_l0.add_(torch.from_numpy(saturating_bias(H)).float())
    gen = torch.Generator().manual_seed(11)
    xs = torch.rand(T, N, I, generator=gen) * 6.0 - 3.0
    resets = torch.rand(T, N, generator=gen) < 0.2
    return rnn, xs, resets


def test_overflow_free_sigmoid_leaves_the_lstm_reference_where_it_was(monkeypatch):
    """``_sigmoid`` through tanh against the textbook 1 / (1 + exp(-v)) it replaced, on the inputs of the GPU tests (default weights, ``x``
    in [-3, 3], 24 steps from a zero state with resets): no result of ``lstm_step64`` moves by more than 1e-15.  At |v| = 1e4 the new form
    is exactly 0 / 1 and raises no warning."""
    rnn, xs, resets = _lstm_case(False, T=24)
    p = lstm_params64(rnn)

    def run():
        h = c = np.zeros((xs.shape[1], 64))
        out = []
        for t in range(xs.shape[0]):
            h, c = lstm_step64(p, xs[t].numpy(), h, c, resets[t].numpy())
            out += [h, c]
        return np.stack(out)

    new = run()
    monkeypatch.setattr(recurrent_ref, "_sigmoid", lambda v: 1.0 / (1.0 + np.exp(-v)))
    old = run()
    moved = float(np.abs(new - old).max())
    print(f"lstm_step64, tanh-form against exp-form sigmoid over 24 steps: max move {moved:.3e}")
    assert moved <= 1e-15 and float(np.abs(old).max()) > 0.5
    monkeypatch.undo()
    with np.errstate(all="raise"):
        s = recurrent_ref._sigmoid(np.array([-1e4, -800.0, 0.0, 800.0, 1e4]))
    assert s.tolist() == [0.0, 0.0, 0.5, 1.0, 1.0]


@pytest.mark.parametrize("saturate", [False, True], ids=["default", "saturated"])
def test_lstm_reference_agrees_with_a_float64_nn_lstm(saturate):
    """``lstm_step64`` against a ``.double()`` copy of ``nn.LSTM`` stepped with ``Memory.reset`` semantics (a reset row starts from zeros),
    to 1e-12; with the saturating biases (pre-activations up to 1e4) nothing overflows and every value stays finite."""
    import copy
    rnn, xs, resets = _lstm_case(saturate)
    rnn64, p = copy.deepcopy(rnn).double(), lstm_params64(rnn)
    N, H = xs.shape[1], 64
    h = c = np.zeros((N, H))
    th, tc = torch.zeros(1, N, H, dtype=torch.float64), torch.zeros(1, N, H, dtype=torch.float64)
    worst = 0.0
    with torch.no_grad(), np.errstate(over="raise", invalid="raise"):
        for t in range(xs.shape[0]):
            h, c = lstm_step64(p, xs[t].numpy(), h, c, resets[t].numpy())
            keep = (~resets[t]).double().view(1, N, 1)
            _, (th, tc) = rnn64(xs[t].double().unsqueeze(0), (th * keep, tc * keep))
            worst = max(worst, float(np.abs(h - th[0].numpy()).max()), float(np.abs(c - tc[0].numpy()).max()))
    print(f"lstm_step64 against nn.LSTM.double(), saturate {saturate}: max diff {worst:.3e}, max |c| {float(np.abs(c).max()):.2f}")
    assert np.isfinite(h).all() and np.isfinite(c).all() and worst < 1e-12
    if saturate:
        assert (h[:, 4::8] == 0.0).all() and np.abs(c[:, 2::8] - 1.0).max() < 1e-11      # o at -1e4; i at +1e4, f at -1e4, g at +30


def test_actor_reference_agrees_with_a_float64_sequential():
    """``actor_forward64`` from explicit arrays against a ``.double()`` copy of the actor ``nn.Sequential`` to 1e-12, with biases in [-1, 1],
    at default weights and at weights x 3 (both ELU branches taken in every layer)."""
    import copy
    torch.manual_seed(2)
    ac = ActorCriticRecurrent(7, 7, 5, actor_hidden_dims=[32, 64, 32], critic_hidden_dims=[16, 16, 16], rnn_hidden_size=32)
    gen = torch.Generator().manual_seed(3)
    h = torch.rand(9, 32, generator=gen) * 2.0 - 1.0
    for gain in (1.0, 3.0):
        with torch.no_grad():
            for m in ac.actor:
                if isinstance(m, torch.nn.Linear):
                    m.weight.mul_(gain)
                    m.bias.copy_(torch.rand(m.bias.shape, generator=gen) * 2.0 - 1.0)
            want = copy.deepcopy(ac.actor).double()(h.double()).numpy()
        w, b = actor_params64(ac.actor)
        assert [x.shape for x in w] == [(32, 32), (64, 32), (32, 64), (5, 32)]
        got = actor_forward64(w, b, h.numpy())
        print(f"actor_forward64 against Sequential.double(), gain {gain}: max diff {float(np.abs(got - want).max()):.3e}, scale {float(np.abs(want).max()):.2f}")
        assert got.shape == (9, 5) and np.abs(got - want).max() < 1e-12
        pre = h.double().numpy() @ w[0].T + b[0]
        assert (pre < -0.5).any() and (pre > 0.5).any()


def _mlp64(seq, x):
    x = np.asarray(x, np.float64)
    for m in seq:
        if isinstance(m, torch.nn.Linear):
            x = x @ m.weight.detach().double().numpy().T + m.bias.detach().double().numpy()
        else:
            x = np.where(x > 0, x, np.expm1(np.minimum(x, 0)))       # ELU
    return x


def _collect(alg, env, T):
    obs = env.get_observations()
    with torch.inference_mode():
        for _ in range(T):
            actions = alg.act(obs, obs)
            obs, _, rew, dones, infos = env.step(actions)
            alg.process_env_step(rew, dones, infos)
    return obs


def _scripted(N, T):
    pattern = torch.zeros(2 * T, N, dtype=torch.bool)
    pattern[0, 0] = True
    pattern[3, 1] = pattern[4, 1] = True
    pattern[T - 1, 2] = True                                 # a done on the last step of the first rollout
    pattern[T + 2, 3] = pattern[T + 5, 0] = True
    pattern[2 * T - 1, 4] = True                             # ... and of the second
    return pattern


def test_batch_mode_replays_two_consecutive_rollouts():
    """Storage, masks and carried state together: the second rollout starts from a non-zero state (zero for the env that was done on the
    first one's last step), and batch-mode evaluation must still reproduce what the rollout stored."""
    N, T, I, A = 6, 8, 5, 3
    ac = _policy(I=I, Ic=I, A=A)
    alg = PPO(ac, num_mini_batches=2, device="cpu")
    alg.init_storage(N, T, [I], [None], [A])
    env = StubEnv(N, I, A, _scripted(N, T))
    for rollout in range(2):
        _collect(alg, env, T)
        st = alg.storage
        if rollout == 1:
            h0 = st.initial_hidden_a[0]
            assert float(h0[0, 2].abs().sum()) == 0.0 and float(h0[0, 5].abs().sum()) > 0.0
        seen = 0
        with torch.no_grad():
            for i, (obs, cobs, act, val, adv, ret, lp, mu, sig, (hid_a, hid_c), masks) in enumerate(st.recurrent_mini_batch_generator(2, 1)):
                assert act.shape == (T, N // 2, A) and obs.shape[0] == T and obs.shape[1] == masks.shape[1] == hid_a[0].shape[1]
                ac.act(obs, masks=masks, hidden_states=hid_a)
                new_lp = ac.get_actions_log_prob(act)
                new_val = ac.evaluate(cobs, masks=masks, hidden_states=hid_c)
                assert (ac.action_mean - mu).abs().max() < 1e-5, (rollout, i)
                assert (new_val - val).abs().max() < 1e-5, (rollout, i)
                assert (new_lp - lp.squeeze(-1)).abs().max() < 1e-5, (rollout, i)
                seen += 1
        assert seen == 2
        st.clear()


def test_trajectory_counts_shapes_and_dropped_tail():
    T, N, I, A = 6, 5, 4, 2
    ac = _policy(I=I, Ic=I, A=A)
    alg = PPO(ac, device="cpu")
    alg.init_storage(N, T, [I], [None], [A])
    st = alg.storage
    st.observations.copy_(torch.arange(T * N * I, dtype=torch.float32).view(T, N, I))
    st.dones.zero_()
    st.dones[1, 0] = 1; st.dones[3, 0] = 1                   # env 0: three trajectories (2, 2, 2)
    st.dones[5, 1] = 1                                       # env 1: one (a done on the last step adds none)
    st.dones[0, 2] = 1; st.dones[1, 2] = 1                   # env 2: three (1, 1, 4)
    st.dones[2, 4] = 1                                       # env 4: two -- and is dropped by 5 // 2 = 2 envs per mini-batch
    st.save_initial_hidden_states(((torch.ones(1, N, 8), 2 * torch.ones(1, N, 8)), None))
    padded, masks = split_and_pad_trajectories(st.observations, st.dones)
    assert padded.shape == (T, 10, I) and masks.sum(0).tolist() == [2, 2, 2, 6, 1, 1, 4, 6, 3, 3]
    assert torch.equal(unpad_trajectories(padded, masks), st.observations)
    batches = list(st.recurrent_mini_batch_generator(2, 1))
    assert len(batches) == 2
    (obs0, _, act0, *_rest0, (hid_a0, hid_c0), m0), (obs1, _, act1, *_rest1, (hid_a1, _), m1) = batches
    assert obs0.shape == (T, 4, I) and m0.shape == (T, 4) and act0.shape == (T, 2, A)             # envs 0, 1: 3 + 1 trajectories
    assert obs1.shape == (T, 4, I) and m1.shape == (T, 4) and act1.shape == (T, 2, A)             # envs 2, 3: 3 + 1
    assert hid_c0 is None and hid_a0[0].shape == (1, 4, 8)
    assert hid_a0[0][0, :, 0].tolist() == [1.0, 0.0, 0.0, 1.0] and hid_a0[1][0, :, 0].tolist() == [2.0, 0.0, 0.0, 2.0]
    assert hid_a1[0][0, :, 0].tolist() == [1.0, 0.0, 0.0, 1.0]
    assert torch.equal(obs0[:2, 1], st.observations[2:4, 0]) and float(obs0[2:, 1].abs().sum()) == 0.0   # env 0's second piece, zero padding behind it
    assert sum(len(list(st.recurrent_mini_batch_generator(2, 3))) for _ in range(1)) == 6


@pytest.mark.parametrize("schedule", ["fixed", "adaptive"])
def test_update_trains_the_memories(schedule):
    N, T, I, A = 6, 8, 5, 3
    ac = _policy(I=I, Ic=I, A=A)
    alg = PPO(ac, num_learning_epochs=2, num_mini_batches=2, schedule=schedule, desired_kl=1e-6, learning_rate=1e-3, device="cpu")
    alg.init_storage(N, T, [I], [None], [A])
    env = StubEnv(N, I, A, _scripted(N, T))
    last = _collect(alg, env, T)
    carried = [t.clone() for t in ac.memory_c.hidden_states]
    with torch.inference_mode():
        alg.compute_returns(last)
    assert all(torch.equal(a, b) for a, b in zip(carried, ac.memory_c.hidden_states))        # the last value does not advance the critic's memory
    before = {k: v.clone() for k, v in ac.state_dict().items()}
    v_loss, s_loss = alg.update()
    assert np.isfinite(v_loss) and np.isfinite(s_loss)
    after = ac.state_dict()
    for k in ("memory_a.rnn.weight_ih_l0", "memory_a.rnn.weight_hh_l0", "memory_c.rnn.weight_ih_l0", "memory_c.rnn.bias_hh_l0"):
        assert not torch.equal(before[k], after[k]), k
    if schedule == "adaptive":
        assert alg.learning_rate < 1e-3                      # any KL is above 2 x 1e-6: the rate went down
    else:
        assert alg.learning_rate == 1e-3


def _train_cfg(name="ActorCriticRecurrent"):
    return {"runner": {"policy_class_name": name, "num_steps_per_env": 8, "save_interval": 50},
            "algorithm": {"num_learning_epochs": 1, "num_mini_batches": 2},
            "policy": {"actor_hidden_dims": [16, 16, 16], "critic_hidden_dims": [16, 16, 16], "rnn_type": "lstm", "rnn_hidden_size": 8, "rnn_num_layers": 1}}


def test_runner_learns_saves_and_loads(tmp_path):
    N, I, A = 6, 5, 3
    torch.manual_seed(0)
    runner = OnPolicyRunner(StubEnv(N, I, A, _scripted(N, 8)), _train_cfg(), log_dir=None, device="cpu")
    assert isinstance(runner.alg.actor_critic, ActorCriticRecurrent) and runner._fused is None
    before = runner.alg.actor_critic.memory_a.rnn.weight_hh_l0.clone()
    runner.learn(2)
    assert not torch.equal(before, runner.alg.actor_critic.memory_a.rnn.weight_hh_l0)
    path = os.path.join(tmp_path, "model_2.pt")
    runner.save(path)
    other = OnPolicyRunner(StubEnv(N, I, A, _scripted(N, 8)), _train_cfg(), log_dir=None, device="cpu")
    other.load(path)
    a, b = runner.alg.actor_critic.state_dict(), other.alg.actor_critic.state_dict()
    assert list(a) == KEYS and all(torch.equal(a[k], b[k]) for k in a) and other.current_learning_iteration == 2
    policy = other.get_inference_policy()
    assert policy(torch.zeros(N, I)).shape == (N, A)
    with pytest.raises(NotImplementedError, match="ActorCriticTransformer"):
        OnPolicyRunner(StubEnv(N, I, A, _scripted(N, 8)), _train_cfg("ActorCriticTransformer"), log_dir=None, device="cpu")


def test_export_and_flags(tmp_path):
    from legged_games_gym_amd.envs.configs import LeggedRobotCfgPPO
    from legged_games_gym_amd.utils.helpers import apply_policy_args, class_to_dict, export_policy_as_jit, get_args
    ac = _policy()
    target = export_policy_as_jit(ac, str(tmp_path))
    assert os.path.basename(target) == "policy_lstm_1.pt"
    mod = torch.jit.load(target)
    xs = torch.rand(10, 1, 5, generator=torch.Generator().manual_seed(2)) * 6.0 - 3.0
    with torch.no_grad():
        want = [ac.act_inference(x) for x in xs]
        got = [mod(x) for x in xs]
        for t in range(10):
            assert (want[t] - got[t]).abs().max() < 1e-6, t
        assert (want[0] - got[1]).abs().max() > 1e-4         # the state matters
        mod.reset_memory()
        assert (mod(xs[0]) - want[0]).abs().max() < 1e-6
    with pytest.raises(NotImplementedError, match="LSTM"):
        export_policy_as_jit(_policy(rnn_type="gru"), str(tmp_path))
    args = get_args(["--policy_class_name", "ActorCriticRecurrent", "--rnn_type", "gru", "--rnn_hidden_size", "64", "--rnn_num_layers", "2"])
    assert (args.policy_class_name, args.rnn_type, args.rnn_hidden_size, args.rnn_num_layers) == ("ActorCriticRecurrent", "gru", 64, 2)
    none = get_args([])
    assert none.policy_class_name is None and none.rnn_type is None and none.rnn_hidden_size is None and none.rnn_num_layers is None
    cfg = apply_policy_args(LeggedRobotCfgPPO(), args)
    d = class_to_dict(cfg)
    assert d["runner"]["policy_class_name"] == "ActorCriticRecurrent" and d["policy"]["rnn_hidden_size"] == 64 and d["policy"]["rnn_type"] == "gru"
    fresh = class_to_dict(LeggedRobotCfgPPO())
    assert not any(k.startswith("rnn_") for k in fresh["policy"]) and fresh["runner"]["policy_class_name"] == "ActorCritic"

    class UserCfg(LeggedRobotCfgPPO):                        # the reference's three lines uncommented in a user subclass
        class policy(LeggedRobotCfgPPO.policy):
            rnn_type = "lstm"
            rnn_hidden_size = 32
            rnn_num_layers = 1

        class runner(LeggedRobotCfgPPO.runner):
            policy_class_name = "ActorCriticRecurrent"
            num_steps_per_env = 4
    user = class_to_dict(UserCfg())
    runner = OnPolicyRunner(StubEnv(4, 5, 3, torch.zeros(4, 4, dtype=torch.bool)), user, log_dir=None, device="cpu")
    assert runner.alg.actor_critic.memory_a.rnn.hidden_size == 32


def test_dec_game_runner_refuses_a_recurrent_policy():
    import types
    from legged_games_gym_amd.rl import DecGamePolicyRunner
    cfg = _train_cfg()
    with pytest.raises(NotImplementedError, match="ActorCriticRecurrent"):
        DecGamePolicyRunner(types.SimpleNamespace(_outcome=None), cfg, log_dir=None, device="cpu")       # refused before anything is built
