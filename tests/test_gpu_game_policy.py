"""-m gpu: ``high_level_game`` on the device path -- the 19-512-256-128-6 actor through ``lg_policy_act``, ``lg_game_act`` (both actors and the
command clip in one launch) against the separate launches it replaces, ``HighLevelGame.step_policy`` / ``make_graphed_policy_step`` against
their parts, and the runner's device rollout against the same launches issued eagerly.  Nothing here reads outside the tree."""
import math

import numpy as np
import pytest
import torch

from tests import game_twin as tw
from tests.game_fixtures import game_registered  # noqa: F401
from tests.test_gpu_game import make_game, pack_params, place_ahead, write_ll_checkpoint

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HIDDEN = [512, 256, 128]


def high_level_actor(seed=3, std=None, bias=None):
    from legged_games_gym_amd.rl import ActorCritic
    torch.manual_seed(seed)
    ac = ActorCritic(19, 19, 6, actor_hidden_dims=HIDDEN, critic_hidden_dims=HIDDEN).to(DEV)
    with torch.no_grad():
        if std is not None:
            ac.std.copy_(torch.as_tensor(std))
        if bias is not None:
            ac.actor[-1].bias.copy_(torch.as_tensor(bias))
    return ac


# ----------------------------------------------------------------------------- 1. the new lg_policy_act shape
@pytest.mark.parametrize("precision", [1, 0])
def test_game_actor_shape_matches_torch_forward(precision):
    """The checks of test_fused_actor_matches_torch_forward on the 19-512-256-128-6 actor: 1e-4 of the output scale at wide precision 1
    (split-bf16 products), 2e-5 at precision 0 (f32 MFMA); N = 1000 leaves a ragged last workgroup at both."""
    from legged_games_gym_amd import capi
    from legged_games_gym_amd.rl import FusedActor
    lib = capi.load_library()
    tol = 2e-5 if precision == 0 else 1e-4
    old = lib.lg_mlp_wide_set_precision(precision)
    try:
        ac = high_level_actor(std=torch.linspace(0.3, 1.4, 6))
        fa = FusedActor(ac, DEV, seed=5)
        obs = torch.randn(1000, 19, device=DEV) * 2.0
        with torch.no_grad():
            want = ac.actor(obs)
        actions, mean = fa.act_with_mean(obs)
        actions, mean = actions.clone(), mean.clone()
        torch.cuda.synchronize()
        scale = float(want.abs().max())
        print(f"precision {precision}: max |mean - torch| = {float((mean - want).abs().max()):.3e}, scale {scale:.3f}")
        assert float((mean - want).abs().max()) < tol * max(1.0, scale)
        z = ((actions - mean) / ac.std.detach()).flatten()
        assert abs(float(z.mean())) < 0.03 and abs(float(z.std()) - 1.0) < 0.03 and float(z.abs().max()) < 6.0
        assert not torch.equal(fa.act(obs).clone(), actions)                       # fresh noise per call
        assert torch.allclose(fa.act_inference(obs), want, atol=tol * max(1.0, scale))
        with torch.no_grad():                                                      # sync() re-uploads changed weights
            ac.actor[0].weight.mul_(0.5)
        fa.sync()
        with torch.no_grad():
            want2 = ac.actor(obs)
        assert torch.allclose(fa.act_inference(obs), want2, atol=tol * max(1.0, float(want2.abs().max())))
        with torch.no_grad():                                                      # sync_device() follows them on the device
            for prm in ac.actor.parameters():
                prm.add_(0.05 * torch.randn_like(prm))
        fa.sync_device()
        want3 = ac.act_inference(obs).detach()
        got3 = fa.act_inference(obs).clone()
        assert float((got3 - want3).abs().max()) < tol * max(1.0, float(want3.abs().max()))
        assert torch.equal(FusedActor(ac, DEV, seed=5).act_inference(obs), got3)   # = a fresh host-side pack
    finally:
        lib.lg_mlp_wide_set_precision(old)


# ----------------------------------------------------------------------------- 2. lg_game_act = the separate launches
# last-layer biases and stds that put every clipped column on both sides of its range (|x| <= 1 for columns 0 / 1, <= 2 for 4 / 5) and
# column 2 on both sides of +pi, with |z| small enough that the f32 log-prob keeps 2e-5
BIAS = (0.7, -0.7, 2.2, 0.0, 1.5, -1.5)
STD = (0.6, 0.6, 1.0, 1.0, 1.0, 1.0)


@pytest.mark.parametrize("counter_on_device", [False, True])
@pytest.mark.parametrize("heading", [1, 0])
@pytest.mark.parametrize("n", [1, 31, 33, 1000, 2000, 4096])
def test_shared_actor_launch_is_bit_identical_to_the_separate_launches(n, heading, counter_on_device):
    from legged_games_gym_amd import capi
    from legged_games_gym_amd.rl import ActorCritic, FusedActor
    lib = capi.load_library()
    assert lib.lg_mlp_wide_set_precision(1) == 1                                   # the default
    hl_ac = high_level_actor(seed=3, std=STD, bias=BIAS)
    torch.manual_seed(4)
    ll_ac = ActorCritic(235, 235, 12, actor_hidden_dims=HIDDEN, critic_hidden_dims=HIDDEN).to(DEV)
    hl, ll = FusedActor(hl_ac, DEV, seed=11), FusedActor(ll_ac, DEV, seed=1)
    gen = torch.Generator().manual_seed(100 + n)
    hl_obs = (torch.randn(n, 19, generator=gen) * 3.0).to(DEV)
    ll_obs = (torch.randn(n, 235, generator=gen) * 1.5).to(DEV)
    P = pack_params(tw.params(num_envs=n, heading_command=heading))
    stream = torch.cuda.current_stream().cuda_stream
    step_value = 77 + n
    counter = torch.tensor([step_value - 1], dtype=torch.int64, device=DEV)        # the kernels read counter + 1
    step, ctr = (-1, counter.data_ptr()) if counter_on_device else (step_value, None)
    seed = 4242

    # the separate launches
    sample_w, mean_w = torch.empty(n, 6, device=DEV), torch.empty(n, 6, device=DEV)
    assert lib.lg_policy_act(hl.handle, hl_obs.data_ptr(), sample_w.data_ptr(), mean_w.data_ptr(), n, seed, step, ctr, 0, stream) == 0
    command_w, llc_w = sample_w.clone(), torch.full((n, 4), 7.0, device=DEV)
    capi.game_pre(P, capi.game_buffers({"command": command_w.data_ptr(), "ll_commands": llc_w.data_ptr()}), stream)
    act_w = torch.empty(n, 12, device=DEV)
    assert lib.lg_policy_act(ll.handle, ll_obs.data_ptr(), act_w.data_ptr(), None, n, seed, step, ctr, 1, stream) == 0

    # one launch
    f = lambda *s: torch.full(s, -9.0, device=DEV)
    command, llc, act, mean, sample, sigma, logp, ocopy = f(n, 6), f(n, 4), f(n, 12), f(n, 6), f(n, 6), f(n, 6), f(n), f(n, 19)
    B = capi.game_buffers({"command": command.data_ptr(), "ll_commands": llc.data_ptr()})
    rc = capi.game_act(hl.handle, ll.handle, P, B, hl_obs.data_ptr(), ll_obs.data_ptr(), act.data_ptr(), mean.data_ptr(), seed, step, ctr, False,
                       sample.data_ptr(), sigma.data_ptr(), logp.data_ptr(), ocopy.data_ptr(), stream)
    assert rc == 0
    torch.cuda.synchronize()
    for name, got, want in (("command", command, command_w), ("ll_commands", llc, llc_w), ("mean", mean, mean_w), ("sample", sample, sample_w),
                            ("ll_actions", act, act_w), ("obs_copy", ocopy, hl_obs), ("ll_commands = command[:, :4]", llc, command[:, :4])):
        assert torch.equal(got, want), (name, float((got - want).abs().max()))
    assert int(counter[0]) == step_value - 1
    std = hl_ac.std.detach()
    assert torch.equal(sigma, std.expand(n, 6))
    want_lp = torch.distributions.Normal(mean, std.expand(n, 6)).log_prob(sample).sum(-1)
    err = float((logp - want_lp).abs().max())
    print(f"n {n} heading {heading}: max |log_prob - torch| = {err:.3e}")
    assert err < 2e-5
    if n >= 1000:                                                                  # both sides of every range, column 2 beyond +-pi
        for col, hi in ((0, 1.0), (1, 1.0), (4, 2.0), (5, 2.0)):
            out = sample[:, col].abs() > hi
            assert bool(out.any()) and bool((~out).any()), col
            assert bool((command[out][:, col].abs() == hi).all()) and torch.equal(command[~out][:, col], sample[~out][:, col])
        beyond = sample[:, 2].abs() > math.pi
        assert bool(beyond.any()) and bool((~beyond).any())
        if heading:
            assert bool((command[beyond][:, 2].abs() <= math.pi).all()) and not torch.equal(command[:, 2], sample[:, 2])
        else:
            assert torch.equal(command[:, 2], sample[:, 2])
    assert torch.equal(command[:, 3], sample[:, 3])

    # the optional outputs are optional; deterministic: the command is the clipped mean
    command2, llc2, act2, mean2 = f(n, 6), f(n, 4), f(n, 12), f(n, 6)
    B2 = capi.game_buffers({"command": command2.data_ptr(), "ll_commands": llc2.data_ptr()})
    assert capi.game_act(hl.handle, ll.handle, P, B2, hl_obs.data_ptr(), ll_obs.data_ptr(), act2.data_ptr(), mean2.data_ptr(), seed, step, ctr, False,
                         stream=stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(command2, command) and torch.equal(llc2, llc) and torch.equal(act2, act) and torch.equal(mean2, mean)
    assert capi.game_act(hl.handle, ll.handle, P, B2, hl_obs.data_ptr(), ll_obs.data_ptr(), act2.data_ptr(), mean2.data_ptr(), seed, step, ctr, True,
                         stream=stream) == 0
    det = mean.clone()
    capi.game_pre(P, capi.game_buffers({"command": det.data_ptr(), "ll_commands": llc_w.data_ptr()}), stream)
    torch.cuda.synchronize()
    assert torch.equal(command2, det) and torch.equal(mean2, mean)


def test_shared_actor_launch_matches_float64_forwards():
    """k_prey_act against references computed outside any kernel, at the smallest size with a second workgroup per role (n = 33): the
    high-level means and the deterministic low-level actions are float64 forwards (``actor_forward64`` from the modules' arrays) of the two
    actors, within 1e-4 of the output scale, the bar of the split-bf16 actors (tests/test_gpu_env_surface.py)."""
    from legged_games_gym_amd import capi
    from legged_games_gym_amd.rl import ActorCritic, FusedActor
    from tests.recurrent_ref import actor_forward64, actor_params64
    assert capi.load_library().lg_mlp_wide_set_precision(1) == 1
    n = 33
    hl_ac = high_level_actor(seed=3, std=STD, bias=BIAS)
    torch.manual_seed(4)
    ll_ac = ActorCritic(235, 235, 12, actor_hidden_dims=HIDDEN, critic_hidden_dims=HIDDEN).to(DEV)
    hl, ll = FusedActor(hl_ac, DEV, seed=11), FusedActor(ll_ac, DEV, seed=1)
    gen = torch.Generator().manual_seed(133)
    hl_obs, ll_obs = (torch.randn(n, 19, generator=gen) * 3.0).to(DEV), (torch.randn(n, 235, generator=gen) * 1.5).to(DEV)
    f = lambda *s: torch.full(s, float("nan"), device=DEV)
    command, llc, act, mean = f(n, 6), f(n, 4), f(n + 5, 12), f(n + 5, 6)
    B = capi.game_buffers({"command": command.data_ptr(), "ll_commands": llc.data_ptr()})
    assert capi.game_act(hl.handle, ll.handle, pack_params(tw.params(num_envs=n)), B, hl_obs.data_ptr(), ll_obs.data_ptr(), act.data_ptr(), mean.data_ptr(),
                         4242, 110, None, False, stream=torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(act[n:]).all()) and bool(torch.isnan(mean[n:]).all())
    for name, got, ac, obs in (("high-level mean", mean[:n], hl_ac, hl_obs), ("low-level actions", act[:n], ll_ac, ll_obs)):
        want = actor_forward64(*actor_params64(ac.actor), obs.cpu().double().numpy())
        err, scale = float(np.abs(got.cpu().double().numpy() - want).max()), max(1.0, float(np.abs(want).max()))
        print(f"[observed] k_prey_act n {n} {name}: err {err:.3e}, scale {scale:.3f}")
        assert err < 1e-4 * scale, (name, err, scale)


def test_shared_actor_launch_refuses_precision_0_and_other_shapes():
    from legged_games_gym_amd import capi
    from legged_games_gym_amd.rl import ActorCritic, FusedActor
    lib = capi.load_library()
    n = 64
    hl, other = FusedActor(high_level_actor(), DEV, seed=1), None
    torch.manual_seed(4)
    ll = FusedActor(ActorCritic(235, 235, 12, actor_hidden_dims=HIDDEN, critic_hidden_dims=HIDDEN).to(DEV), DEV, seed=1)
    other = FusedActor(ActorCritic(48, 48, 12, actor_hidden_dims=[128, 64, 32], critic_hidden_dims=[128, 64, 32]).to(DEV), DEV, seed=1)
    t = {k: torch.zeros(n, w, device=DEV) for k, w in (("command", 6), ("llc", 4), ("act", 12), ("mean", 6), ("hl_obs", 19), ("ll_obs", 235))}
    P = pack_params(tw.params(num_envs=n))
    B = capi.game_buffers({"command": t["command"].data_ptr(), "ll_commands": t["llc"].data_ptr()})
    call = lambda a, b: capi.game_act(a.handle, b.handle, P, B, t["hl_obs"].data_ptr(), t["ll_obs"].data_ptr(), t["act"].data_ptr(), t["mean"].data_ptr(),
                                      1, 1, None, False, stream=torch.cuda.current_stream().cuda_stream)
    assert call(hl, ll) == 0
    assert call(hl, other) == -4 and call(ll, ll) == -4
    old = lib.lg_mlp_wide_set_precision(0)
    try:
        assert call(hl, ll) == -4
    finally:
        lib.lg_mlp_wide_set_precision(old)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- 3. / 4. the env surface
def two_games(tmp_path, seed, reset_seed):
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    N = 512
    A, B = make_game(ckpt, N, seed=seed), make_game(ckpt, N, seed=seed)
    timed = torch.arange(0, 32, device=DEV)
    for env in (A, B):
        torch.manual_seed(reset_seed)             # reset_idx from the host draws from torch's generator
        env.reset()
        place_ahead(env, torch.arange(32, 64, device=DEV), 0.8)
        env.ll_env.episode_length_buf[timed] = int(env.ll_env.max_episode_length) - 12
    return A, B


def assert_same_state(A, B, k):
    for name in ("obs_buf", "rew_buf", "reset_buf", "predator_pos", "curr_episode_step"):
        assert torch.equal(getattr(A, name), getattr(B, name)), (k, name)
    assert torch.equal(A.ll_env.root_states, B.ll_env.root_states) and torch.equal(A.ll_env.obs_buf, B.ll_env.obs_buf), k
    assert torch.equal(A.ll_env.commands, B.ll_env.commands), k


@pytest.mark.parametrize("precision", [1, 0])
def test_step_policy_equals_actor_then_step(tmp_path, precision):
    """A: ``step_policy(fused_a)``.  B, identically seeded: ``fused_b.act_with_mean(obs)`` then ``step(actions)``.  Same actor seed and step count.
    At wide precision 0 ``step_policy`` takes the separate launches (rc -4) and must agree as well."""
    from legged_games_gym_amd import capi
    from legged_games_gym_amd.rl import FusedActor
    lib = capi.load_library()
    old = lib.lg_mlp_wide_set_precision(precision)
    try:
        A, B = two_games(tmp_path, seed=9, reset_seed=90)
        ac = high_level_actor(seed=6)
        fa, fb = FusedActor(ac, DEV, seed=21), FusedActor(ac, DEV, seed=21)
        resets, clipped, inside = 0, 0, 0
        sample = torch.empty(A.num_envs, 6, device=DEV)
        for k in range(30):
            prev_a = A.obs_buf
            (ca, ma), (oa, _, ra, da, _) = A.step_policy(fa, sample=sample)
            actions, mb = fb.act_with_mean(B.obs_buf)
            raw = actions.clone()
            ob, _, rb, db, _ = B.step(actions)                         # clips `actions` where it is
            torch.cuda.synchronize()
            assert torch.equal(ca, actions) and torch.equal(ma, mb) and torch.equal(sample, raw), k
            assert oa is A.obs_buf and oa is not prev_a and torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db), k
            assert_same_state(A, B, k)
            assert A.ll_env.common_step_counter == B.ll_env.common_step_counter and A._obs_flip == B._obs_flip
            resets += int(da.sum()); clipped += int((raw != ca).sum()); inside += int((raw == ca).all(dim=1).sum())
        assert resets >= 32 and clipped > 0 and inside > 0, (resets, clipped, inside)
    finally:
        lib.lg_mlp_wide_set_precision(old)


def test_graphed_policy_step_equals_eager_step_policy(tmp_path):
    """``make_graphed_policy_step`` (3 warm-up steps, then 20 replays of the three captured launches) equals 23 eager ``step_policy`` calls."""
    from legged_games_gym_amd.rl import FusedActor
    A, B = two_games(tmp_path, seed=9, reset_seed=90)
    ac = high_level_actor(seed=6)
    fa = FusedActor(ac, DEV, seed=21, step_counter=A.ll_env._sim.buf["step_counter"])
    fb = FusedActor(ac, DEV, seed=21, step_counter=B.ll_env._sim.buf["step_counter"])
    with pytest.raises(ValueError):
        A.make_graphed_policy_step(FusedActor(ac, DEV, seed=21))                   # a host-counted noise stream cannot be replayed
    replay = A.make_graphed_policy_step(fa, warmup=3)
    for _ in range(3):
        B.step_policy(fb)
    assert A.ll_env.common_step_counter == B.ll_env.common_step_counter
    resets = 0
    for k in range(20):
        oa, _, ra, da, _ = replay()
        (cb, mb), (ob, _, rb, db, _) = B.step_policy(fb)
        torch.cuda.synchronize()
        ca, ma = fa.output_buffers(A.num_envs)
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db) and torch.equal(ca, cb) and torch.equal(ma, mb), k
        assert_same_state(A, B, k)
        for env in (A, B):
            assert int(env.ll_env._sim.buf["step_counter"][0]) == env.ll_env.common_step_counter
        resets += int(da.sum())
    assert resets >= 32 and A.ll_env.common_step_counter == B.ll_env.common_step_counter


# ----------------------------------------------------------------------------- 5. the runner
def game_runner(reg, tmp_path, monkeypatch, ckpt, n, device_rollout=True, **runner_keys):
    import legged_games_gym_amd.utils.task_registry as tr_mod
    from legged_games_gym_amd.utils import get_args
    monkeypatch.setattr(tr_mod, "LEGGED_GYM_ROOT_DIR", str(tmp_path))
    env_cfg, train_cfg = reg.get_cfgs("high_level_game")
    env_cfg.terrain.mesh_type, env_cfg.env.ll_policy_path = "plane", ckpt
    for key in ("device_rollout", "graphed_rollout"):
        if hasattr(train_cfg.runner, key):
            delattr(train_cfg.runner, key)
    if device_rollout:
        train_cfg.runner.device_rollout = True                          # a runner key, not a config field: set on this registration only
    for key, value in runner_keys.items():
        setattr(train_cfg.runner, key, value)
    args = get_args(["--task", "high_level_game", "--num_envs", str(n), "--headless", "--sim_device", DEV, "--rl_device", DEV])
    env, _ = reg.make_env("high_level_game", args)
    torch.manual_seed(1234)                                              # the same initial actor / critic on every runner
    runner, _ = reg.make_alg_runner(env, "high_level_game", args)
    return env, runner


def test_runner_device_rollout_captured_equals_eager_and_keeps_the_generic_storage_semantics(tmp_path, monkeypatch, game_registered):
    reg = game_registered
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    N = 512
    env_g, run_g = game_runner(reg, tmp_path, monkeypatch, ckpt, N)
    env_e, run_e = game_runner(reg, tmp_path, monkeypatch, ckpt, N, graphed_rollout=False)
    assert run_g._fused is not None and run_e._fused is not None and run_g._game_rollout and not hasattr(env_g, "_sim")
    assert torch.equal(env_g.obs_buf, env_e.obs_buf) and env_g.common_step_counter == env_e.common_step_counter
    T = run_g.num_steps_per_env
    # captured: one eager warm-up rollout (discarded), then the capture, then one replay
    graphed = run_g._try_build_graphed_rollout()
    assert graphed is not None and run_e._try_build_graphed_rollout() is None
    graph, _, obs_g, _ = graphed
    with torch.inference_mode():
        graph.replay()
    env_g.common_step_counter += T
    # eager: the same two rollouts as plain launches
    sums = torch.zeros(3, device=DEV)
    stats = {"cur_rew": torch.zeros(N, device=DEV), "cur_len": torch.zeros(N, device=DEV), "sum_rew": sums[0], "sum_len": sums[1], "count": sums[2], "_sums": sums}
    with torch.inference_mode():
        run_e._rollout_steps(stats)
        obs_e, _ = run_e._rollout_steps(stats)
    torch.cuda.synchronize()
    sg, se = run_g.alg.storage, run_e.alg.storage
    for name in ("observations", "actions", "mu", "sigma", "actions_log_prob", "rewards", "dones", "values"):
        assert torch.equal(getattr(sg, name), getattr(se, name)), name
    assert torch.equal(obs_g, obs_e) and obs_g is env_g.obs_buf and env_g.common_step_counter == env_e.common_step_counter
    assert int(env_g.ll_env._sim.buf["step_counter"][0]) == env_g.common_step_counter
    assert int(sg.dones.sum()) > 0 and torch.isfinite(sg.values).all() and float(sg.values.abs().max()) > 0

    # storage semantics of the generic path: clipped commands, log-prob / sigma of the unclipped sample
    P = env_g._P
    act, mu, sigma, lp = sg.actions, sg.mu, sg.sigma, sg.actions_log_prob[..., 0]
    for col, rng in ((0, P.cmd_lin_vel_x), (1, P.cmd_lin_vel_y), (4, P.predator_lin_vel_x), (5, P.predator_lin_vel_y)):
        assert float(act[..., col].min()) >= rng[0] and float(act[..., col].max()) <= rng[1]
    assert P.heading_command == 1 and float(act[..., 2].abs().max()) <= math.pi + 1e-6
    assert torch.equal(sigma, run_g.alg.actor_critic.std.detach().expand_as(sigma))
    # the unclipped samples are not stored: draw them again (same weights, seed and step keys; lg_policy_act is bit-identical to the actor launch)
    lib, fused = run_e._fused.lib, run_e._fused
    stream = torch.cuda.current_stream().cuda_stream
    sample, mean = torch.empty_like(act), torch.empty_like(mu)
    for t in range(T):
        step = env_g.common_step_counter - T + t + 1
        assert lib.lg_policy_act(fused.handle, sg.observations[t].data_ptr(), sample[t].data_ptr(), mean[t].data_ptr(), N, fused.seed, step, None, 0, stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(mean, mu)
    want = torch.from_numpy(np.stack([tw.pre(tw.params(num_envs=N, heading_command=1), sample[t].cpu().numpy())[0] for t in range(T)])).to(DEV)
    assert torch.equal(act, want)                                        # the stored action is the clipped / wrapped sample
    lp_of_sample = torch.distributions.Normal(mu, sigma).log_prob(sample).sum(-1)
    lp_of_stored = torch.distributions.Normal(mu, sigma).log_prob(act).sum(-1)
    assert float((lp - lp_of_sample).abs().max()) < 2e-5                 # ... and the stored log-prob is the sample's, on every row
    # a clip is active where the sample lies outside the column's range, the wrap where |sample| > pi in column 2 (inside (-pi, pi] the wrap
    # is the identity up to the rounding of (a + 2 pi) - 2 pi on negative values: 2 ulp of 2 pi, 1e-6)
    active = sample[..., 2].abs() > math.pi
    for col, rng in ((0, P.cmd_lin_vel_x), (1, P.cmd_lin_vel_y), (4, P.predator_lin_vel_x), (5, P.predator_lin_vel_y)):
        active |= (sample[..., col] < rng[0]) | (sample[..., col] > rng[1])
    assert float((sample - act)[~active].abs().max()) <= 1e-6
    diff = (lp - lp_of_stored).abs()
    # On an active row the stored log-prob is NOT that of the stored action.  Two kinds of active row cannot show it: a clip that moves the
    # action by less than the f32 resolution of the log-prob, and one that mirrors the action about the mean (possible only where the mean
    # itself lies beyond the range end), which leaves the density unchanged.  Rows with a column that moved by more than 1e-3 and whose
    # distance from the mean changed by more than 1e-3 are free of both and must differ by more than the 2e-5 allowed on untouched rows.
    # The rest of the active rows: a sample within 1e-3 of a range end has probability < 1e-3 x the peak density 0.4 per clipped column, a
    # mirror within 1e-3 the same order -- a few rows in a thousand; 2 % of the active rows is the bound, ten times that.
    moved = ((sample - act).abs() > 1e-3) & (((sample - mu).abs() - (act - mu).abs()).abs() > 1e-3)
    clear = active & moved.any(dim=-1)
    n_active, n_clear = int(active.sum()), int(clear.sum())
    print(f"rows: {lp.numel()}  clip or wrap active {n_active} (clearly moved {n_clear})  untouched {int((~active).sum())}  "
          f"max diff untouched {float(diff[~active].max()):.3e}  min diff clearly moved {float(diff[clear].min()):.3e}  "
          f"active rows within 2e-5: {int((diff[active] <= 2e-5).sum())}")
    # both kinds of row are present (an untrained actor on observations that still hold the +-100 fill values puts most means outside the ranges:
    # far fewer than the four rows in ten that zero means would leave untouched)
    assert int((~active).sum()) > 0 and n_active > 0 and n_clear > 0
    assert float(diff[~active].max()) < 2e-5
    assert float(diff[clear].min()) > 2e-5
    assert n_active - n_clear <= 0.02 * n_active and int((diff[active] <= 2e-5).sum()) <= 0.02 * n_active


def test_runner_device_rollout_learns_saves_and_plays(tmp_path, monkeypatch, game_registered):
    from legged_games_gym_amd.scripts.play import play
    from legged_games_gym_amd.utils import get_args
    from legged_games_gym_amd.utils.helpers import get_load_path
    reg = game_registered
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    env, runner = game_runner(reg, tmp_path, monkeypatch, ckpt, 512)
    losses = []
    update = runner.alg.update
    runner.alg.update = lambda *a, **k: losses.append(update(*a, **k)) or losses[-1]
    before = [p.detach().clone() for p in runner.alg.actor_critic.actor.parameters()]
    runner.learn(num_learning_iterations=3, init_at_random_ep_len=True)
    torch.cuda.synchronize()
    assert len(losses) == 3 and all(math.isfinite(float(v)) for pair in losses for v in pair)
    assert any(not torch.equal(a, b) for a, b in zip(before, runner.alg.actor_critic.actor.parameters()))
    obs = env.get_observations()
    # the device actor followed the optimiser (sync_device after every update)
    want = runner.alg.actor_critic.act_inference(obs).detach()
    got = runner._fused.act_inference(obs)
    assert float((got - want).abs().max()) < 1e-4 * max(1.0, float(want.abs().max()))
    assert torch.isfinite(obs).all() and torch.isfinite(env.rew_buf).all()
    path = get_load_path(str(tmp_path / "logs" / "high_level_game_flat"))
    assert path.endswith("model_3.pt")
    env2 = play(get_args(["--task", "high_level_game", "--headless", "--sim_device", DEV, "--rl_device", DEV]), steps=5)
    assert env2.num_envs == 50 and torch.isfinite(env2.obs_buf).all()


def test_runner_switch_off_keeps_the_generic_loop(tmp_path, monkeypatch, game_registered):
    reg = game_registered
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    env, runner = game_runner(reg, tmp_path, monkeypatch, ckpt, 64, device_rollout=False)
    assert runner._fused is None and runner._game_rollout is False
    calls = []
    step_policy = env.step_policy
    env.step_policy = lambda *a, **k: calls.append(1) or step_policy(*a, **k)
    runner.learn(num_learning_iterations=1)
    assert not calls                                                    # eager generic loop: PPO.act -> env.step -> process_env_step
