"""-m gpu: Cassie's step kernels (k_step<CassieTraits, PD, plane | HF, NW = 4 / 2 / 1>) against the oracle through landing, stance and
fall -- toes on the ground, joints beyond their hard limits and at the speed limit, pelvis contact, the -200 termination term, the
in-step reset and the terrain-level change, in a full 32-env workgroup and in the 8 live lanes of a partial one.

The trajectory, its action schedule and its event masks are those of tests/cassie_fall.py; tests/test_cassie_fall.py proves on the CPU
that the run visits these branches and that no flag of it sits on a rounding edge.  Every compared step is ONE policy step from the
oracle's own state, copied whole into the device buffers: chaotic divergence never enters.
"""
import types

import numpy as np
import pytest
import torch

from tests import cassie_fall as F
from tests.test_gpu_full_size import _compare_every_env, _get, _spawn

pytestmark = pytest.mark.gpu

N, T = F.N, F.T
DEV = "cuda:0"
BUDGET = dict(pos_tol=2e-3, vel_tol=0.3, obs_tol=2e-2, rew_tol=2e-3)      # test_cassie_heightfield_step_parity's (config 5's) budget


def _device(s):
    from legged_games_gym_amd.device_sim import DeviceSim
    if s["terr"] is None:
        return DeviceSim(s["p"], s["model"], s["robot"], torch.device(DEV), s["w"])
    return DeviceSim(s["p"], s["model"], s["robot"], torch.device(DEV), s["w"], s["terr"].heightsamples, s["terr"].env_origins)


def _oracle_to_device(state, d):
    """Every buffer of an oracle snapshot into the device's: the reverse of tests/test_gpu_full_size._device_to_oracle."""
    for name, val in state.items():
        t = d.buf[name]
        t.copy_(torch.from_numpy(np.ascontiguousarray(val)).to(t.dtype).view(t.shape))


def _waves(N_envs):
    """tests/test_gpu_step_variants._waves with Cassie's 32 envs per workgroup."""
    wg, C = (N_envs + F.WORKGROUP_ENVS - 1) // F.WORKGROUP_ENVS, torch.cuda.get_device_properties(0).multi_processor_count
    return 4 if wg <= C else (2 if wg <= 2 * C else 1)


@pytest.mark.parametrize("kind", F.KINDS)
def test_every_step_of_the_fall_against_the_oracle(kind):
    """N = 40 (NW = 4, a full workgroup and one with 8 live envs), all 48 steps, each from the oracle's recorded state with the recorded
    actions and counter, every env compared.
    Bit-equal on every env and step: reset_buf, time_out_buf, episode_length_buf, terrain_levels, last_contacts.
    Survivors, pooled over the 1920 env-steps: joint positions and root pose within 2e-3, joint and root velocities within 0.3 (the budget
    of test_cassie_heightfield_step_parity); at most 2 env-steps (0.1 %, the rule of _compare_every_env) may leave it and must stay
    within 20 x; medians below tol / 50.  On the env-steps inside the budget: rew_buf and episode_sums 2e-3, obs_buf 2e-2 (height field:
    on the envs whose measured_heights agree, as _compare_every_env; at most 0.2 % of the samples may not), feet_air_time 1e-6,
    contact_forces 2e-3 of the step's largest force, base row included.
    Reset envs: rew_buf within 2e-3 of the oracle's (-200 dt dominates it) and the re-drawn state (root_states, dof_state, commands,
    env_origins, feet_air_time, last_actions, last_dof_vel, episode_sums) within 1e-6.
    Nothing new is bounded here, and the kernels are far inside the budget: their distance from the oracle is that of the oracle from
    itself under one ulp of input noise (tests/test_cassie_fall.py: 6e-6 rad, 4.5e-4 rad/s).  The bounds stay where they are.
    [observed] plane: 1890 survivors and 30 resets in 1920 env-steps; worst joint position 3.5e-6, joint velocity 3.2e-4, root pose 9.5e-7,
    root velocity 5.8e-5; medians 3.6e-7 / 2.5e-5; 0 env-steps outside the budget; rew_buf 4.7e-7, episode_sums 4.5e-7, obs_buf 1.6e-5,
    feet_air_time 0, contact_forces 5.5e-5 of the largest; reset envs: rew_buf 4.8e-7, re-drawn state 7.2e-7.
    height field: 1890 survivors and 30 resets; worst joint position 4.2e-6, joint velocity 3.4e-4, root pose 1.9e-6, root velocity
    6.1e-5; medians 3.6e-7 / 2.7e-5; 0 env-steps outside the budget; rew_buf 6.8e-7, episode_sums 7.3e-7, obs_buf 1.8e-5, feet_air_time
    0, contact_forces 3.9e-5 of the largest; reset envs: rew_buf 4.8e-7, re-drawn state 4.8e-7; measured_heights 0 of 228690 samples apart."""
    tr = F.trajectory(kind)
    s = tr["setup"]
    d = _device(s)
    if kind == "heightfield":
        # the restated terrain and spawn are those of the tests they are taken from: same samples, same state after the spawn
        from tests.test_gpu_parity import _rough_terrain
        assert np.array_equal(_rough_terrain(N).heightsamples, s["terr"].heightsamples)
        _spawn(d, N, s["terr"], s["cfg"], np.random.default_rng(0), (0.5, 1.25), (-1.0, 1.0))
        for k in ("friction_coeffs", "base_mass_delta", "terrain_levels", "terrain_types", "env_origins", "root_states", "dof_state"):
            assert np.array_equal(_get(d, k), tr["states"][0][k]), k
    assert _waves(N) == 4
    pooled = {k: [] for k in ("pos", "vel", "root", "rv")}
    worst = dict(rew=0.0, sums=0.0, obs=0.0, air=0.0, force=0.0, reset_rew=0.0, reset_state=0.0)
    inside_checks, mh_mismatch, mh_total, resets = [], 0, 0, 0
    for t in range(1, T + 1):
        ref = tr["states"][t]
        _oracle_to_device(tr["states"][t - 1], d)
        d.step(torch.from_numpy(tr["actions"][t - 1]).to(DEV), t)
        assert d.sim.device_status(True) == 0
        dev = {k: _get(d, k) for k in ref}
        for k in F.FLAGS:
            if k in ref:
                assert np.array_equal(ref[k], dev[k]), (k, t, np.nonzero((ref[k] != dev[k]).reshape(N, -1).any(axis=1))[0])
        alive = ref["reset_buf"] == 0
        q_o, q_d = ref["dof_state"].reshape(N, 12, 2).astype(np.float64), dev["dof_state"].reshape(N, 12, 2).astype(np.float64)
        r_o, r_d = ref["root_states"].astype(np.float64), dev["root_states"].astype(np.float64)
        e = dict(pos=np.abs(q_o[..., 0] - q_d[..., 0]).max(axis=1), vel=np.abs(q_o[..., 1] - q_d[..., 1]).max(axis=1),
                 root=np.abs(r_o[:, :7] - r_d[:, :7]).max(axis=1), rv=np.abs(r_o[:, 7:] - r_d[:, 7:]).max(axis=1))
        for k in pooled:
            pooled[k].append(e[k][alive])
        inside = alive & (e["pos"] < BUDGET["pos_tol"]) & (e["root"] < BUDGET["pos_tol"]) & (e["vel"] < BUDGET["vel_tol"]) & (e["rv"] < BUDGET["vel_tol"])
        diff = lambda k: np.abs(ref[k].astype(np.float64) - dev[k].astype(np.float64))
        same_cells = inside
        if "measured_heights" in ref:
            mism = diff("measured_heights") > 1e-6
            mh_mismatch, mh_total = mh_mismatch + int(mism[alive].sum()), mh_total + int(mism[alive].size)
            same_cells = inside & ~mism.any(axis=1)
        f_scale = max(1.0, float(np.abs(ref["contact_forces"]).max()))
        step_e = dict(rew=diff("rew_buf")[inside].max(initial=0.0), sums=diff("episode_sums")[:, inside].max(initial=0.0),
                      obs=diff("obs_buf")[same_cells].max(initial=0.0), air=diff("feet_air_time")[inside].max(initial=0.0),
                      force=diff("contact_forces")[inside].max(initial=0.0) / f_scale)
        gone = ~alive
        if gone.any():
            resets += int(gone.sum())
            step_e["reset_rew"] = diff("rew_buf")[gone].max()
            step_e["reset_state"] = max(diff(k).reshape(N, -1)[gone].max() for k in ("root_states", "dof_state", "commands", "env_origins", "feet_air_time", "last_actions", "last_dof_vel"))
            step_e["reset_state"] = max(step_e["reset_state"], diff("episode_sums")[:, gone].max())
        inside_checks.append((t, step_e))
        worst = {k: max(v, float(step_e.get(k, 0.0))) for k, v in worst.items()}
    pooled = {k: np.concatenate(v) for k, v in pooled.items()}
    outside = ((pooled["pos"] >= BUDGET["pos_tol"]) | (pooled["root"] >= BUDGET["pos_tol"]) | (pooled["vel"] >= BUDGET["vel_tol"]) | (pooled["rv"] >= BUDGET["vel_tol"]))
    print(f"[observed] {kind}: survivors {pooled['pos'].size} of {T * N} env-steps, resets {resets}; worst joint position {pooled['pos'].max():.3g}, joint velocity {pooled['vel'].max():.3g}, "
          f"root pose {pooled['root'].max():.3g}, root velocity {pooled['rv'].max():.3g}; medians {np.median(pooled['pos']):.3g} / {np.median(pooled['vel']):.3g}; "
          f"env-steps outside the budget {int(outside.sum())}; inside it: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items())
          + (f"; measured_heights samples apart {mh_mismatch} of {mh_total}" if mh_total else ""))
    assert outside.sum() <= 2, int(outside.sum())
    assert pooled["pos"].max() < 20 * BUDGET["pos_tol"] and pooled["root"].max() < 20 * BUDGET["pos_tol"]
    assert pooled["vel"].max() < 20 * BUDGET["vel_tol"] and pooled["rv"].max() < 20 * BUDGET["vel_tol"]
    assert np.median(pooled["pos"]) < BUDGET["pos_tol"] / 50 and np.median(pooled["vel"]) < BUDGET["vel_tol"] / 50
    if mh_total:
        assert mh_mismatch < 2e-3 * mh_total, (mh_mismatch, mh_total)
    for t, e in inside_checks:
        assert e["rew"] < BUDGET["rew_tol"] and e["sums"] < BUDGET["rew_tol"] and e["obs"] < BUDGET["obs_tol"], (t, e)
        assert e["air"] < 1e-6 and e["force"] < 2e-3, (t, e)
        assert e.get("reset_rew", 0.0) < BUDGET["rew_tol"] and e.get("reset_state", 0.0) < 1e-6, (t, e)
    assert resets >= 10


@pytest.mark.parametrize("n_of_c", [(32, 8), (64, 8)], ids=["32C+8", "64C+8"])
def test_landing_stance_and_fall_with_fewer_helper_waves(n_of_c):
    """The plane run at 32 C + 8 envs (NW = 2) and 64 C + 8 envs (NW = 1), C compute units, each with an 8-env last workgroup.  Three steps
    chosen from the oracle alone -- the first with at least 30 % of the envs on a toe, step 16, and the first from 20 on in which at
    least 0.5 % of the envs reset -- each from the oracle's state, compared by _compare_every_env at the budget above; min_contact_frac 0
    for the landing step, the oracle's own share minus 0.05 for the other two.
    [observed] with C = 256: the chosen steps are 8, 16 and 21 at both sizes.  Landing: 13 % of the envs on one toe, 19 % on two, 32 % with
    more than 50 N; stance: 99.6 % on two toes; fall: 13 % on one toe, 79 % on two, 77 resets of 8200 and 144 of 16392 (none of them in the
    last workgroup: its resets are the N = 40 test's).  Worst surviving env, joint position / velocity (envs outside the budget):
    N = 8200 landing 2.6e-6 / 3.9e-4 (0), stance 2.2e-3 / 0.44 (1), fall 7.8e-6 / 1.7e-3 (0); N = 16392 landing 8.0e-3 / 0.42 (1), stance
    2.9e-6 / 4.2e-4 (0), fall 1.4e-2 / 0.12 (1).  The single envs outside are inside 20 x and within the 0.1 % that _compare_every_env
    allows a branch taken on an ulp; everywhere else the kernels are three orders inside the budget."""
    N_envs = n_of_c[0] * torch.cuda.get_device_properties(0).multi_processor_count + n_of_c[1]
    assert _waves(N_envs) == {32: 2, 64: 1}[n_of_c[0]] and N_envs % F.WORKGROUP_ENVS == 8
    s, chosen = F.chosen_steps(N_envs, threads=16)
    d = _device(s)
    for name in ("landing", "stance", "fall"):
        c = chosen[name]
        _oracle_to_device(c["before"], d)
        d.step(torch.from_numpy(c["actions"]).to(DEV), c["step"])
        assert d.sim.device_status(True) == 0
        after = c["after"]
        cf = after["contact_forces"].reshape(N_envs, -1, 3)
        toes = (cf[:, s["robot"].bodies_matching("toe"), 2] > 1.0).sum(axis=1)
        q_o, q_d = after["dof_state"].reshape(N_envs, 12, 2), _get(d, "dof_state").reshape(N_envs, 12, 2)
        alive = after["reset_buf"] == 0
        e_pos, e_vel = np.abs(q_o[..., 0] - q_d[..., 0]).max(axis=1), np.abs(q_o[..., 1] - q_d[..., 1]).max(axis=1)
        print(f"[observed] N = {N_envs} {name}: step {c['step']}, one toe {float((toes == 1).mean()):.3f}, two toes {float((toes == 2).mean()):.3f}, F_z > 50 N {c['contact_share']:.3f}, "
              f"resets {int(after['reset_buf'].sum())} ({int(after['reset_buf'][-8:].sum())} in the last workgroup); worst joint position {e_pos[alive].max():.3g}, "
              f"joint velocity {e_vel[alive].max():.3g}, envs outside the budget {int((alive & ((e_pos >= BUDGET['pos_tol']) | (e_vel >= BUDGET['vel_tol']))).sum())}")
        frac = 0.0 if name == "landing" else c["contact_share"] - 0.05
        _compare_every_env(types.SimpleNamespace(buf=after), lambda k: _get(d, k), N_envs, c["step"], min_contact_frac=frac, **BUDGET)
