"""-m gpu: the fused policy kernels against the CPU oracle, every step and every env.

The rollout kernel (lg_rollout_policy: k_step<Anymal, NET, plane, POL, NW 4, SC, ROLL>, the launch bench.py times) and the fused policy
step (lg_step_policy: the same without ROLL) on anymal_c_flat with the flat task's random-init PPO actor, as bench.py sets it up.
A segment of T = 20 steps (bench's --graph-steps) starts from a settled state whose episode lengths put time-outs on every step and
whose counter puts the push step inside the segment.  S_t is the state after t steps: S_0 is a snapshot, S_k (k < 20) the final
state of a k-step launch from S_0, S_20 that of the 20-step launch.  Each step is checked three ways:
- a segment's first k steps do not depend on its length (storage slices bit-equal to the 20-step launch's);
- the oracle, loaded with S_t and given the kernel's actions[t], reproduces S_{t+1} within the one-step budget of
  tests/test_gpu_full_size.py (config 3's bounds), flags bit-equal.  Over 20 steps x 4096 envs a contact onset or a stick / slide
  switch taken on a 1-ulp difference inside the bulk is met a few times (the single-step kernel from the same S_t gives bit-identical
  forces): contact forces take the joint states' rule (99.9 % of the bulk envs within the budget, the rest 20x), and the actuator
  hidden state, rewards and observations are compared on the bulk envs whose joint velocities agree within 0.01 rad/s, which must
  be all but 0.1 % of the bulk;
- mean[t] is a float64 forward of the actor on obs[t], and actions[t] - mean[t] is std * eps of tests/philox_np.action_noise.

The exploration noise of the stand-alone actor kernels (lg_policy_act: the f32 kernel and k_policy_act_wide) is checked against the
same independent reference (tests/noise_check.py, which states the tolerances).
"""
import copy

import numpy as np
import pytest
import torch

from tests.common import make_setup, grid_origins, randomize_env_params
from tests.noise_check import check_noise as _check_noise
from tests.test_gpu_full_size import _compare_every_env

pytestmark = pytest.mark.gpu

T = 20                       # bench.py --graph-steps
C0 = 740                     # first step's counter: the push step (counter % 750 == 0) is step t = 10 of the segment
TOLS = dict(vel_tol=0.1, pos_tol=1e-3, obs_tol=1e-2, rew_tol=1e-3)      # config 3's every-env budget
NO_COMPARE = ("episode_means", "extras_accum")     # float atomics; roll_finish publishes only the segment's last resetting step


def _flat_setup(N, sc):
    from oracle.oracle import OracleSim
    from legged_games_gym_amd.device_sim import DeviceSim
    from legged_games_gym_amd.envs import task_registry
    from legged_games_gym_amd.rl import ActorCritic, FusedActor
    from legged_games_gym_amd.utils.helpers import class_to_dict
    cfg, robot, p, names, model, w = make_setup("anymal_c_flat", N, tweak=lambda c: setattr(c.asset, "self_collisions", 0 if sc else 1))
    assert p.self_collision == int(sc) and p.push_interval == 750 and p.num_obs == 48
    o = OracleSim(p, model, robot, w, threads=16)
    d = DeviceSim(p, model, robot, torch.device("cuda:0"), w)
    _, train_cfg = task_registry.get_cfgs("anymal_c_flat")
    torch.manual_seed(train_cfg.seed)                                  # bench.py: random-init policy
    ac = ActorCritic(p.num_obs, p.num_obs, 12, **class_to_dict(train_cfg.policy)).cuda()
    fa = FusedActor(ac, "cuda:0", seed=train_cfg.seed)
    fr, dm = randomize_env_params(N, 5)
    d.buf["env_origins"].copy_(torch.from_numpy(grid_origins(N)))
    d.buf["friction_coeffs"].copy_(torch.from_numpy(fr)); d.buf["base_mass_delta"].copy_(torch.from_numpy(dm))
    d.reset_idx(torch.arange(N, dtype=torch.int32), 0)
    z = torch.zeros(N, 12, device="cuda")
    for it in range(1, 9):                                             # settle onto the plane
        d.step(z, it)
    # time-outs on every step of the segment: an env with episode length L times out at step 1000 - L
    rng = np.random.default_rng(N)
    L = rng.integers(0, 950, N)
    late = rng.random(N) < 0.3
    L[late] = 981 + rng.integers(0, 20, int(late.sum()))
    if N < 20:
        L[0], L[-1] = 990, 981                                         # first env and the partial workgroup's last one
    d.buf["episode_length_buf"].copy_(torch.from_numpy(L).to(d.buf["episode_length_buf"].dtype))
    d.buf["step_counter"].fill_(C0 - 1)
    return robot, p, o, d, ac, fa


def _snap(d):
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in d.buf.items()}


def _restore(d, S):
    for k, v in S.items():
        d.buf[k].copy_(v)


def _np(t):
    return (t.to(torch.uint8) if t.dtype == torch.bool else t).cpu().numpy()


def _storage(steps, N):
    f = lambda *s: torch.full(s, float("nan"), device="cuda")         # a slot the kernel does not write stays NaN
    return {"obs": f(steps + 1, N, 48), "actions": f(steps, N, 12), "mean": f(steps, N, 12), "rew": f(steps, N),
            "dones": torch.zeros(steps, N, dtype=torch.bool, device="cuda"), "time_outs": torch.zeros(steps, N, dtype=torch.bool, device="cuda")}


def _launch(d, fa, S0, steps, counter):
    _restore(d, S0)
    st = _storage(steps, d.params.num_envs)
    d.rollout_policy(fa, st, counter, obs0=d.buf["obs_buf"])
    assert d.sim.device_status(True) == 0                             # no missed LDS hand-over
    return st, _snap(d)


def _state_to_oracle(o, S, obs):
    for name, dst in o.buf.items():
        dst[...] = _np(S[name]).astype(dst.dtype).reshape(dst.shape)
    o.buf["obs_buf"][...] = obs                                        # the rollout writes observations to its storage only


def _check_oracle_step(o, S_t, S_next, obs_t, obs_next, actions, rew, dones, time_outs, step, N, report):
    """One step of the oracle from S_t with the kernel's actions against the kernel's S_{t+1} and storage slices."""
    _state_to_oracle(o, S_t, obs_t)
    o.step(actions, step)
    dev = lambda k: obs_next if k == "obs_buf" else _np(S_next[k])
    # dense time-outs keep up to ~40 % of the robots in the air (re-spawned above the ground, ~0.3 s to land): contact share 0.5
    survivors, bulk = _compare_every_env(o, dev, N, step, min_contact_frac=0.5, same_branch_vel=0.01, **TOLS)
    assert np.array_equal(o.buf["reset_buf"], dones.astype(o.buf["reset_buf"].dtype))
    assert np.array_equal(o.buf["time_out_buf"], time_outs.astype(o.buf["time_out_buf"].dtype))
    assert np.abs(o.buf["rew_buf"] - rew)[bulk].max() < TOLS["rew_tol"]
    assert np.abs(o.buf["obs_buf"] - obs_next)[bulk].max() < TOLS["obs_tol"]
    e_h = float(np.abs(o.buf["sea_hidden_state"] - dev("sea_hidden_state")).reshape(2, N, -1)[:, bulk].max())
    assert e_h < 5e-3, e_h                                             # config 3's bound, on the envs that took the same branches
    q_o, q_d = o.buf["dof_state"].reshape(N, 12, 2), dev("dof_state").reshape(N, 12, 2)
    report["dof_pos"] = max(report.get("dof_pos", 0.0), float(np.quantile(np.abs(q_o[..., 0] - q_d[..., 0]).max(axis=1), 0.999)))
    report["dof_vel"] = max(report.get("dof_vel", 0.0), float(np.quantile(np.abs(q_o[..., 1] - q_d[..., 1]).max(axis=1), 0.999)))
    report["rew"] = max(report.get("rew", 0.0), float(np.abs(o.buf["rew_buf"] - rew)[bulk].max()))
    report["obs"] = max(report.get("obs", 0.0), float(np.abs(o.buf["obs_buf"] - obs_next)[bulk].max()))
    report["sea_hidden"] = max(report.get("sea_hidden", 0.0), e_h)


def _check_actor(ac, fa, obs, mean, actions, step, report):
    """mean: float64 forward of a float64 copy of the actor (2e-5 of the output scale); actions - mean: std * eps of the reference."""
    actor64 = copy.deepcopy(ac.actor).double().cpu()
    with torch.no_grad():
        want = actor64(torch.from_numpy(obs).double()).numpy()
    scale = max(1.0, float(np.abs(want).max()))
    e_mean = float(np.abs(mean.astype(np.float64) - want).max())
    assert e_mean < 2e-5 * scale, (e_mean, scale)
    report["mean_rel"] = max(report.get("mean_rel", 0.0), e_mean / scale)
    _check_noise(actions, mean, ac.std.detach().double().cpu().numpy(), fa.seed, step, report)


@pytest.mark.parametrize("sc", [True, False], ids=["sc_on", "sc_off"])
@pytest.mark.parametrize("N", [4096, 4100, 5])
def test_rollout_kernel_against_the_oracle_every_step(N, sc):
    """4096: the bench size, one workgroup of 16 envs per CU; 4100: 257 workgroups, the last one with 4 envs (dead lanes alias env N - 1);
    5: one partial workgroup.  Storage slices of the k-step launches are bit-equal to the 20-step launch's; episode_means and the
    extras slots are excluded: roll_finish publishes only the segment's last resetting step, so they depend on the length."""
    robot, p, o, d, ac, fa = _flat_setup(N, sc)
    S0 = _snap(d)
    st20, S20 = _launch(d, fa, S0, T, C0)
    roll = {k: _np(v) for k, v in st20.items()}
    # time-outs on every step (N >= 4096), at least one in the segment (N = 5); the push step lies inside the segment
    per_step = roll["time_outs"].sum(axis=1)
    assert (per_step >= 8).all() if N >= 4096 else per_step.sum() >= 1, per_step
    assert any((C0 + t) % p.push_interval == 0 for t in range(T))
    S = {0: S0, T: S20}
    for k in range(1, T):
        st_k, S[k] = _launch(d, fa, S0, k, C0)
        for name, v in st_k.items():
            assert np.array_equal(_np(v), roll[name][:k + 1 if name == "obs" else k]), (k, name)
        assert int(S[k]["step_counter"][0]) == C0 + k - 1
    report = {}
    for t in range(T):
        _check_oracle_step(o, S[t], S[t + 1], roll["obs"][t], roll["obs"][t + 1], roll["actions"][t], roll["rew"][t], roll["dones"][t],
                           roll["time_outs"][t], C0 + t, N, report)
        _check_actor(ac, fa, roll["obs"][t], roll["mean"][t], roll["actions"][t], C0 + t, report)
    # the graphed rollout's call (bench, runner): counter -1, the kernel reads step_counter (= C0 - 1) and advances it
    st_dev, S_dev = _launch(d, fa, S0, T, -1)
    for name, v in st_dev.items():
        assert np.array_equal(_np(v), roll[name]), name
    for name, v in S_dev.items():
        if name not in NO_COMPARE:
            assert torch.equal(v, S20[name]), name
    assert int(S_dev["step_counter"][0]) == C0 + T - 1
    # lg_step_policy (the POL instantiation without ROLL) from S_0
    _restore(d, S0)
    actions, mean = d.step_policy(fa, d.buf["obs_buf"], C0)
    assert d.sim.device_status(True) == 0
    actions, mean, obs0 = _np(actions), _np(mean), _np(S0["obs_buf"])
    _check_oracle_step(o, S0, _snap(d), obs0, _np(d.buf["obs_buf"]), actions, _np(d.buf["rew_buf"]), _np(d.buf["reset_buf"]),
                       _np(d.buf["time_out_buf"]), C0, N, report)
    _check_actor(ac, fa, obs0, mean, actions, C0, report)
    print(f"[observed] rollout N={N} sc={sc}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(report.items())))


def test_policy_act_noise_matches_the_reference():
    """lg_policy_act: the f32 kernel (48-128-64-32) at a ragged N, and the 235 / 169-512-256-128 shapes with both
    lg_mlp_wide_set_precision settings (0: the f32 kernel, 1: k_policy_act_wide).  Every build's actions - mean is std * eps of
    tests/philox_np.action_noise for the same (seed, env, step), and the wide kernel's noise equals the f32 kernel's."""
    from legged_games_gym_amd import capi
    from legged_games_gym_amd.rl import ActorCritic, FusedActor
    lib = capi.load_library()
    N, step, report = 1000, 37, {}
    std = torch.linspace(0.3, 1.4, 12)
    old = lib.lg_mlp_wide_set_precision(1)
    try:
        for n_obs, hidden in ((48, [128, 64, 32]), (235, [512, 256, 128]), (169, [512, 256, 128])):
            torch.manual_seed(3)
            ac = ActorCritic(n_obs, n_obs, 12, actor_hidden_dims=hidden, critic_hidden_dims=hidden).cuda()
            with torch.no_grad():
                ac.std.copy_(std)
            obs = torch.randn(N, n_obs, device="cuda") * 2.0
            noise = []
            for precision in ((1,) if n_obs == 48 else (0, 1)):
                lib.lg_mlp_wide_set_precision(precision)
                fa = FusedActor(ac, "cuda:0", seed=5)
                fa._host_step = step - 1                               # _call advances it to `step`
                a, m = (_np(x.clone()) for x in fa.act_with_mean(obs))
                _check_noise(a, m, std.double().numpy(), 5, step, report)
                noise.append((a, m))
            for a, m in noise[1:]:                                     # same samples from both builds for the same (seed, env, step)
                a0, m0 = noise[0]
                diff = np.abs((a.astype(np.float64) - m) - (a0.astype(np.float64) - m0))
                assert (diff <= 1e-6 * (1.0 + np.abs(a) + np.abs(a0))).all(), float(diff.max())
    finally:
        lib.lg_mlp_wide_set_precision(old)
    print("[observed] policy_act noise: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(report.items())))
