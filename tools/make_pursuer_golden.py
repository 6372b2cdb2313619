#!/usr/bin/env python3
"""Generate the scripted-pursuer fixtures under tests/golden/ (run in the build container only; needs the reference tree).

pursuer_step.npz         -- inputs + outputs of the reference's OWN ``HighLevelGame.step`` (high_level_game.py:146-241) with the predator driven by
                            its OWN ``full_obs_predator('integrator')`` (:289-324), on the stand-in objects of tools/make_game_golden.py
                            (``build_objects``; ``full_obs_predator`` is added to the extracted methods).  ONE departure from the reference's text:
                            the stand-in's wrapper around ``step_predator_single_integrator`` drops the ``command`` argument it is called with, so
                            the method takes its ``command=None`` branch.  That is the edit of line 188 with which the reference's users ran the
                            scripted pursuer; the fixture states it under the key ``departure``.  The method bodies are extracted with ``ast`` at
                            generation time (nothing is copied into this repo).  The stand-in's own deliberate difference (``base_quat`` served
                            after the step's resets) is that of game_step.npz.
                            Two sequences of consecutive calls on N = 512 envs, as game_step.npz: ``a`` (env_radius None, 4 calls) and ``b``
                            (env_radius 6, 3 calls); the same recorded arrays plus ``predator_command`` (the velocity the reference used) and
                            ``ep`` (the episode step it was computed from: ``curr_episode_step`` after the increment of :182).
pursuer_provenance.json  -- the SHA-256 of every reference file executed (the format of game_provenance.json).

The predator's move depends on the prey's position, so the prey is drawn first -- relative to the predator BEFORE it moves -- and the redraw
loop of make_game_golden.py clears the threshold margins.  The initial ``curr_episode_step`` is drawn from [0, 1.3 L), and the generator
asserts in every call that at least 5 % of the velocity components are unsaturated, 5 % saturated at a positive limit, and 5 % of the envs
past ``max_episode_length`` (a negative limit: torch.clamp with min > max returns max).  Env 0 is kept occluded and alive, as in game_step.npz."""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import make_golden as mg                                   # noqa: E402
import make_game_golden as gg                              # noqa: E402
from tests import game_twin as tw                          # noqa: E402
from tests import pursuer_twin as pt                       # noqa: E402

N = gg.N
F = np.float32
DEPARTURE = "step_predator_single_integrator is entered with command=None (the argument of high_level_game.py:188 is dropped)"


def record_provenance(*fixtures):
    path = os.path.join(mg.OUT, "pursuer_provenance.json")
    table = json.load(open(path)) if os.path.isfile(path) else {}
    for f in fixtures:
        table[f] = dict(sorted(mg.EXECUTED.items()))
    with open(path, "w") as fh:
        json.dump(dict(sorted(table.items())), fh, indent=1)


def sequence(tag, radius, calls, seed, rng):
    import torch
    origins = gg.grid_origins(N)
    env, ll, draws, ns = gg.build_objects(radius, False, origins)
    for name, fn in mg._ref_functions(gg.HLG, "HighLevelGame", ns, lambda k: k == "full_obs_predator").items():
        setattr(type(env), name, fn)
    p = tw.params(**gg.twin_params(env, ll, seed))
    q = pt.pursuer_params(max_episode_length=int(env.max_episode_length))     # max_lin_vel / min_lin_vel / gain: the literals of :301, :312, :307
    L = q["max_episode_length"]
    pred0 = (origins + np.stack((rng.uniform(-2, 2, N), rng.uniform(-2, 2, N), np.full(N, 0.3)), axis=1)).astype(F)
    state = dict(predator_pos=pred0, obs=np.full((N, 19), 100.0, F), curr_episode_step=rng.integers(0, int(1.3 * L), N).astype(np.int64),
                 episode_length_buf=rng.integers(1, 50, N).astype(np.int64), episode_sums=np.zeros((2, N), F), env_origins=origins)
    ll.root_states[ll.predator_indices, :3] = torch.from_numpy(pred0)
    env.obs_buf = torch.from_numpy(state["obs"]).clone()
    env.rew_buf, env.reset_buf = torch.zeros(N), torch.ones(N, dtype=torch.long)
    env.curr_episode_step = torch.from_numpy(state["curr_episode_step"]).clone()
    env.episode_length_buf = torch.from_numpy(state["episode_length_buf"]).clone()
    env._update_agent_states()
    rec = {k: [] for k in ("in_command", "in_root_states", "in_ll_rew", "in_ll_dones", "step", "u_root", "u_pred", "command", "predator_command", "ep",
                           "predator_integrated", "predator_pos", "root_states", "obs", "rew", "reset_buf", "curr_episode_step", "episode_length_buf",
                           "episode_sums", "sense_pos", "sense_flag")}
    ll.feed = {"root_states": [], "ll_rew": [], "ll_dones": []}
    inner_integrate, inner_policy, inner_sense = type(env).step_predator_single_integrator, type(env).full_obs_predator, type(env).sense_predator
    tap = {}

    def step_predator_single_integrator(self, command=None):
        inner_integrate(self)                                                    # THE departure: ``command`` is dropped (line 188 edited)
        tap["predator_integrated"] = self.predator_pos.clone().numpy()

    def full_obs_predator(self, dyn_type):
        u1, u2 = inner_policy(self, dyn_type)
        tap["predator_command"] = torch.stack((u1, u2), dim=1).clone().numpy()
        tap["ep"] = self.curr_episode_step.clone().numpy()
        return u1, u2

    def sense_predator(self):
        pos, flag = inner_sense(self)
        tap["sense_pos"], tap["sense_flag"] = pos.clone().numpy(), flag[:, 0].clone().numpy()
        return pos, flag
    type(env).step_predator_single_integrator, type(env).full_obs_predator, type(env).sense_predator = step_predator_single_integrator, full_obs_predator, sense_predator

    twin_state = dict(state)
    for k in range(calls):
        # multiples of 1/1024 (the clip and the wrap are game_step.npz's business, and short mantissas keep this file below its size)
        command = (rng.integers(-3072, 3073, (N, 6)) / 1024.0).astype(F)
        command[:, 2] = (rng.integers(-9216, 9217, N) / 1024.0).astype(F)   # beyond +-pi: the wrap of column 2
        clipped, _ = tw.pre(p, command)
        # the prey first, relative to the predator where it stands: the pursuer's move (at most 0.04 m per axis) follows from it
        root, ll_rew, ll_dones = gg.draw_inputs(rng, np.arange(N), twin_state["predator_pos"], origins, radius)
        for attempt in range(40):
            step_key = 1000 * (k + 1) + attempt
            for _ in range(30):
                s = dict(twin_state, command=clipped, root_states=root, ll_rew=ll_rew, ll_reset=ll_dones)
                out, info = pt.post(p, q, s, step=step_key)
                viol = gg.per_env_violations(p, info)
                viol[0] |= bool(info["visible"][0]) or bool(out["reset_buf"][0])        # env 0 stays occluded and alive (make_game_golden.py)
                bad = np.nonzero(viol)[0]
                if len(bad) == 0:
                    break
                r2, w2, d2 = gg.draw_inputs(rng, bad, twin_state["predator_pos"], origins, radius)
                root[bad], ll_rew[bad], ll_dones[bad] = r2, w2, d2
            if len(bad) == 0:
                break
        assert len(bad) == 0, "could not clear the threshold margins"
        tw.assert_margins(p, info)
        unsat, sat, neg = pt.branch_shares(info)
        assert min(unsat, sat, neg) >= 0.05, (tag, k, unsat, sat, neg)
        ll.call = k
        ll.feed["root_states"].append(torch.from_numpy(root).clone())
        ll.feed["ll_rew"].append(torch.from_numpy(ll_rew).clone())
        ll.feed["ll_dones"].append(torch.from_numpy(ll_dones).clone())
        done_ids = np.nonzero(out["reset_buf"])[0]
        draws.begin(seed, step_key, done_ids, False)
        cmd_t = torch.from_numpy(command).clone()
        with gg._patched_torch(draws):
            obs, _, rew, reset_buf, _ = env.step(cmd_t)                          # the reference's own step(), whole
        assert np.array_equal(np.nonzero(reset_buf.numpy())[0], done_ids), "twin and reference disagree on the done envs"
        assert tap["predator_command"].dtype == np.float32
        assert np.array_equal(tap["predator_command"].view(np.uint32), info["predator_command"].view(np.uint32)), "twin and reference disagree on the velocity"
        u_root, u_pred = tw.draws(seed, N, step_key)
        rec["in_command"].append(command); rec["in_root_states"].append(root.copy()); rec["in_ll_rew"].append(ll_rew.copy()); rec["in_ll_dones"].append(ll_dones.copy())
        rec["step"].append(step_key); rec["u_root"].append(u_root); rec["u_pred"].append(u_pred)
        rec["command"].append(cmd_t.numpy().copy()); rec["predator_command"].append(tap["predator_command"]); rec["ep"].append(tap["ep"])
        rec["predator_integrated"].append(tap["predator_integrated"])
        rec["predator_pos"].append(env.predator_pos.clone().numpy()); rec["root_states"].append(ll.root_states[ll.prey_indices].clone().numpy())
        rec["obs"].append(obs.clone().numpy()); rec["rew"].append(rew.clone().numpy()); rec["reset_buf"].append(reset_buf.clone().numpy())
        rec["curr_episode_step"].append(env.curr_episode_step.clone().numpy()); rec["episode_length_buf"].append(env.episode_length_buf.clone().numpy())
        rec["episode_sums"].append(np.stack([env.episode_sums[n_].clone().numpy() for n_ in ("evasion", "pursuit")]))
        rec["sense_pos"].append(tap["sense_pos"]); rec["sense_flag"].append(tap["sense_flag"])
        twin_state = {kk: out[kk] for kk in ("predator_pos", "obs", "curr_episode_step", "episode_length_buf", "episode_sums", "env_origins")}
        cap = info["capture"]
        dist = info["dist_xy"]
        print(f"  {tag} call {k}: step key {step_key}, unsaturated {unsat:.3f}, saturated at a positive limit {sat:.3f}, negative limit {int((info['lim'] < 0).sum())}/{N}, "
              f"prey at {dist.min():.2f}-{dist.max():.2f} m, visible {int(tap['sense_flag'].sum())}, captured {int(cap.sum())}, ll only {int((ll_dones & ~cap).sum())}, "
              f"radius {int(info['radius'].sum())}, neither {int((~out['reset_buf']).sum())}")
    res = {f"{tag}_{k}": np.stack(v) if k != "step" else np.array(v, np.int64) for k, v in rec.items()}
    res.update({f"{tag}_in0_{k}": state[k] for k in ("predator_pos", "obs", "curr_episode_step", "episode_length_buf", "episode_sums")})
    res[f"{tag}_env_origins"] = origins
    res[f"{tag}_params"] = np.array(json.dumps(p))
    res[f"{tag}_pursuer_params"] = np.array(json.dumps(q))
    return res


def step_fixture():
    mg.EXECUTED.clear()
    rng = np.random.default_rng(40)
    out = {}
    out.update(sequence("a", None, 4, seed=21, rng=rng))
    out.update(sequence("b", 6.0, 3, seed=22, rng=rng))
    out["base_quat_source"] = np.array("root_states at read time (after the step's resets)")
    out["env0"] = np.array("occluded and not done in every call")
    out["departure"] = np.array(DEPARTURE)
    path = os.path.join(mg.OUT, "pursuer_step.npz")
    np.savez_compressed(path, **out)
    record_provenance("pursuer_step.npz")
    size, ref = os.path.getsize(path), os.path.getsize(os.path.join(mg.OUT, "game_step.npz"))
    assert size <= ref, f"pursuer_step.npz ({size} bytes) is larger than game_step.npz ({ref} bytes)"
    print(f"pursuer_step.npz written ({size} bytes; game_step.npz {ref})")


if __name__ == "__main__":
    step_fixture()
