#!/usr/bin/env python3
"""Cost of the game layer around the low-level step (GPU only).

Times, with device events around >= 2000 replays after warm-up, alternating in one process, at the registered 2000 envs and at 4096:
  (a) the graphed high-level step (``HighLevelGame.make_graphed_step``) with a random-init 19-512-256-128-6 policy:
      high-level actor, k_game_pre, low-level actor, k_step, k_game_post;
  (b) the same graph without the two game kernels and without the high-level actor (low-level actor + k_step: one `a1` policy step);
  (c) the eager ``step``.
Writes profiles/game_step.json (or --out): the three times per repeat, their spread over the repeats, the overhead (a) - (b) and the
env-steps/s of (a).  ``--trace`` runs a short replay loop only, for ``rocprofv3 --kernel-trace --stats -- python tools/game_probe.py --trace``.

``--policy-step`` times the device path of the high-level actor instead and writes profiles/game_policy_step.json (game_step.json is left alone):
  (p) the three-launch graph (``make_graphed_policy_step``): lg_game_act, k_step, k_game_post;
  (a) the graphed step with the torch actor, as above;
  (s) the five-launch graph with both actors on lg_policy_act: ``make_graphed_step(fused.act)``: lg_policy_act, k_game_pre, lg_policy_act, k_step, k_game_post;
then the step as the runner's device rollout captures it (two ``step_policy`` calls per graph, the observations alternating between two buffers),
per step, with the copy of the observations written by the actor launch and with an ``obs_buf.copy_`` kernel in front of it;
and, unless ``--train-iterations 0``, PPO training of the registered task with the runner's ``device_rollout`` on and off (env-steps/s including the
update, same seed and size).  With ``--trace`` it replays (p) only.

``--scripted`` builds ``scripted_predator_game`` beside ``high_level_game`` in one process and times the graphed three-launch policy step of both
(lg_game_act, k_step, then k_pursuer_post against k_game_post), alternating; writes profiles/pursuer_step.json.

``--outcome`` builds both tasks with the outcome statistics off and on (four envs per size, one process) and times their graphed three-launch
policy step, alternating: k_outcome_post<false> against k_game_post and k_outcome_post<true> against k_pursuer_post in the same run; writes
profiles/game_outcome_step.json.

``--recurrent`` times the recurrent policy's device path (a random-init ``ActorCriticRecurrent``, ``--rnn-hidden`` units per memory, the
512-256-128 actor behind it) and writes profiles/game_recurrent_step.json, per step of a two-step graph (the memories alternate between two
state slots), alternating in one process:
  (r) the four-launch step: lg_lstm_step, lg_game_lstm_act, k_step, k_game_post;
  (s) the same graph with the policy stage as separate launches: lg_lstm_step, lg_lstm_actor_act, k_game_pre, lg_policy_act, k_step, k_game_post;
  (f) the feed-forward three-launch step of the same env: lg_game_act, k_step, k_game_post;
then, unless ``--train-iterations 0``, PPO training with ``ActorCriticRecurrent`` and the runner's ``device_rollout`` on and off: env-steps/s
including the update, and the rollout's and the update's share of an iteration from synchronised stamps around every update.  With ``--trace``
it replays (r) only.  With ``--gru`` a fourth variant joins the alternation, (g) the four-launch step with GRU memories (the key ``device_gru``):
lg_gru_step, lg_game_lstm_act, k_step, k_game_post; no training then, and the file is profiles/game_recurrent_gru_step.json.

The low-level policy is a seeded random-init checkpoint written to a temporary directory: the kernels' cost does not depend on the weights."""
import argparse
import json
import os
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402


DEFAULT_OUT = os.path.join(REPO, "profiles", "game_step.json")


def make_env(n, mesh, tmp, scripted=False):
    from legged_games_gym_amd.envs import task_registry
    from legged_games_gym_amd.envs.a1_game import HighLevelGame, HighLevelGameFlatCfg, ScriptedPredatorGame, ScriptedPredatorGameCfg
    from legged_games_gym_amd.rl import ActorCritic
    from legged_games_gym_amd.utils import get_args, set_seed
    from legged_games_gym_amd.utils.helpers import class_to_dict, parse_sim_params
    a1_cfg, a1_train = task_registry.get_cfgs("a1")
    torch.manual_seed(0)
    ac = ActorCritic(a1_cfg.env.num_observations, a1_cfg.env.num_observations, a1_cfg.env.num_actions, **class_to_dict(a1_train.policy))
    ckpt = os.path.join(tmp, "model_0.pt")
    torch.save({"model_state_dict": ac.state_dict(), "optimizer_state_dict": {}, "iter": 0, "infos": None}, ckpt)
    cfg = ScriptedPredatorGameCfg() if scripted else HighLevelGameFlatCfg()
    cfg.env.num_envs, cfg.env.ll_policy_path, cfg.terrain.mesh_type, cfg.seed = n, ckpt, mesh, 1
    args = get_args(["--headless", "--sim_device", "cuda:0", "--rl_device", "cuda:0"])
    set_seed(1)
    env = (ScriptedPredatorGame if scripted else HighLevelGame)(cfg, parse_sim_params(args, {"sim": class_to_dict(cfg.sim)}), args.physics_engine, "cuda:0", True)
    torch.manual_seed(1)
    hl = ActorCritic(env.num_obs, env.num_obs, env.num_actions, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128]).to("cuda:0").eval()

    def policy(obs):
        with torch.no_grad():
            return hl.act_inference(obs)
    env.reset()
    return env, policy


def graph_low_level_only(env, warmup=3):
    """Low-level actor + lg_step captured the way HighLevelGame.make_graphed_step captures them, without the game."""
    ll = env.ll_env
    sim = ll._sim
    sim.set_obs_output(ll.obs_buf)
    sim.buf["step_counter"].fill_(ll.common_step_counter)
    side = torch.cuda.Stream(device=env.device)
    side.wait_stream(torch.cuda.current_stream(env.device))
    with torch.cuda.stream(side):
        for _ in range(warmup):
            sim.step(env.ll_policy(ll.obs_buf), -1)
            ll.common_step_counter += 1
    torch.cuda.current_stream(env.device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    ll.begin_graph_capture()
    sim.set_deferred_extras(False)
    try:
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            sim.step(env.ll_policy(ll.obs_buf), -1)
    finally:
        ll.end_graph_capture(0)

    def replay():
        graph.replay()
        ll.common_step_counter += 1
    return replay


def fused_high_level_actor(env):
    """The probe's random-init 19-512-256-128-6 actor on the MFMA kernels, its noise keyed by the low-level sim's device step counter."""
    from legged_games_gym_amd.rl import ActorCritic, FusedActor
    torch.manual_seed(1)
    hl = ActorCritic(env.num_obs, env.num_obs, env.num_actions, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128]).to("cuda:0").eval()
    return FusedActor(hl, "cuda:0", seed=7, step_counter=env.ll_env._sim.buf["step_counter"])


def graph_rollout_steps(env, fused, steps, separate_copy):
    """``steps`` (even) ``step_policy`` calls captured the way the runner's device rollout captures them: the observations alternate
    between the two buffers, the actor launch carrying them over.  ``separate_copy``: ``obs_out.copy_(obs_in)`` in front of an actor launch
    that reads and writes ``obs_out`` instead -- what the in-launch copy replaces.  Returns a callable that replays the ``steps`` steps."""
    if separate_copy:
        act = env._act

        def copy_then_act(fa, obs_in, obs_out, *a, **k):
            if obs_out is not obs_in:
                obs_out.copy_(obs_in)
            return act(fa, obs_out, obs_out, *a, **k)
        env._act = copy_then_act
    try:
        for _ in range(steps):
            env.step_policy(fused)
        torch.cuda.synchronize()
        env.begin_graph_capture()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            for _ in range(steps):
                env.step_policy(fused)
            env.capture_extras_flush()
        env.end_graph_capture(steps)
    finally:
        if separate_copy:
            del env._act

    def replay():
        graph.replay()
        env.common_step_counter += steps
    return replay


def train_steps_per_s(n, mesh, tmp, device_rollout, iterations, warm=2, rnn_hidden=None):
    """env-steps/s of ``OnPolicyRunner.learn`` on high_level_game (rollout + update), after ``warm`` iterations that build graphs and workspaces.
    ``rnn_hidden``: train an ``ActorCriticRecurrent`` with that many units per memory."""
    import time
    from legged_games_gym_amd.envs import a1_game, task_registry
    from legged_games_gym_amd.utils import get_args
    from legged_games_gym_amd.utils.helpers import apply_policy_args
    a1_game.register()
    try:
        env_cfg, train_cfg = task_registry.get_cfgs("high_level_game")
        env_cfg.env.ll_policy_path, env_cfg.terrain.mesh_type = os.path.join(tmp, "model_0.pt"), mesh
        if device_rollout:
            train_cfg.runner.device_rollout = True
        args = get_args(["--task", "high_level_game", "--num_envs", str(n), "--headless", "--sim_device", "cuda:0", "--rl_device", "cuda:0", "--seed", "1"]
                        + (["--policy_class_name", "ActorCriticRecurrent", "--rnn_hidden_size", str(rnn_hidden)] if rnn_hidden else []))
        apply_policy_args(train_cfg, args)
        env, _ = task_registry.make_env("high_level_game", args)
        torch.manual_seed(1)
        runner, _ = task_registry.make_alg_runner(env, "high_level_game", args, log_root=None)
        marks = []
        if rnn_hidden:                                 # where an iteration's time goes: synchronised stamps around every update
            update = runner.alg.update

            def stamped_update(*a, **k):
                torch.cuda.synchronize()
                t = time.perf_counter()
                out = update(*a, **k)
                torch.cuda.synchronize()
                marks.append((t, time.perf_counter()))
                return out
            runner.alg.update = stamped_update
        runner.learn(num_learning_iterations=warm)
        torch.cuda.synchronize()
        del marks[:]
        t0 = time.perf_counter()
        runner.learn(num_learning_iterations=iterations)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert (runner._fused is not None) == bool(device_rollout)
        rate = iterations * runner.num_steps_per_env * n / dt
        if not rnn_hidden:
            return rate
        # rollout = from the end of one update to the start of the next (graph replay or the generic loop, returns, the actor's device repack)
        rollouts = [1e3 * (marks[i][0] - marks[i - 1][1]) for i in range(1, len(marks))]
        updates = [1e3 * (b - a) for a, b in marks]
        return {"env_steps_per_s": rate, "rollout_ms": {"median": statistics.median(rollouts), "min": min(rollouts), "max": max(rollouts)},
                "update_ms": {"median": statistics.median(updates), "min": min(updates), "max": max(updates)}}
    finally:
        a1_game.unregister()


def policy_step_main(args):
    result = {"device": torch.cuda.get_device_name(0), "mesh_type": args.mesh, "replays": args.replays, "repeats": args.repeats, "envs": {}, "training": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for n in args.envs:
            env, policy = make_env(n, args.mesh, tmp)
            fused = fused_high_level_actor(env)
            shared = env.make_graphed_policy_step(fused)
            if args.trace:
                for _ in range(200):
                    shared()
                torch.cuda.synchronize()
                continue
            torch_actor = env.make_graphed_step(policy)
            separate = env.make_graphed_step(fused.act)
            for fn in (shared, torch_actor, separate):
                timed(fn, 200)
            p, a, s = [], [], []
            for _ in range(args.repeats):              # alternating: other work shares the machine
                p.append(timed(shared, args.replays))
                a.append(timed(torch_actor, args.replays))
                s.append(timed(separate, args.replays))
            result["envs"][str(n)] = {"graphed_policy_step": spread(p), "graphed_step_torch_actor": spread(a), "graphed_step_separate_actor_launches": spread(s),
                                      "env_steps_per_s_graphed_policy_step": n / (statistics.median(p) * 1e-6)}
            assert torch.isfinite(env.obs_buf).all() and torch.isfinite(env.ll_env.root_states).all()
            print(f"{n} envs: three launches {statistics.median(p):.1f} us, torch actor "
                  f"{statistics.median(a):.1f} us, separate actor launches {statistics.median(s):.1f} us", flush=True)
            # the rollout's form of the step (observations ping-pong): the copy inside the actor launch against a copy kernel in front of it
            in_launch, copy_kernel = graph_rollout_steps(env, fused, 2, False), graph_rollout_steps(env, fused, 2, True)
            for fn in (in_launch, copy_kernel):
                timed(fn, 100)
            ci, ck = [], []
            for _ in range(args.repeats):
                ci.append(timed(in_launch, args.replays // 2) / 2)
                ck.append(timed(copy_kernel, args.replays // 2) / 2)
            result["envs"][str(n)]["rollout_step_copy_in_actor_launch"] = spread(ci)
            result["envs"][str(n)]["rollout_step_separate_copy_kernel"] = spread(ck)
            assert torch.isfinite(env.obs_buf).all() and torch.isfinite(env.ll_env.root_states).all()
            print(f"{n} envs, per step of a captured two-step rollout: copy in the actor launch {statistics.median(ci):.1f} us, "
                  f"copy kernel + actor launch {statistics.median(ck):.1f} us", flush=True)
        if not args.trace and args.train_iterations > 0:
            n = args.envs[0]
            for key, on in (("device_rollout_off", False), ("device_rollout_on", True)):
                result["training"][key] = {"envs": n, "iterations": args.train_iterations,
                                           "env_steps_per_s": train_steps_per_s(n, args.mesh, tmp, on, args.train_iterations)}
                print(f"training, {n} envs, {key}: {result['training'][key]['env_steps_per_s']:.0f} env-steps/s", flush=True)
    if not args.trace:
        out = args.out if args.out != DEFAULT_OUT else os.path.join(REPO, "profiles", "game_policy_step.json")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as fh:
            json.dump(result, fh, indent=1)
        print("wrote", out)


def recurrent_main(args):
    """The recurrent policy's graphed step against the same graph with the policy stage as separate launches and against the feed-forward
    three-launch step, per step of a two-step graph; then training with the runner's switch on and off."""
    from legged_games_gym_amd.rl import ActorCriticRecurrent
    from legged_games_gym_amd.rl.recurrent_actor import RecurrentFusedActor
    result = {"device": torch.cuda.get_device_name(0), "mesh_type": args.mesh, "replays": args.replays, "repeats": args.repeats,
              "rnn_hidden_size": args.rnn_hidden, "steps_per_replay": 2, "envs": {}, "training": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for n in args.envs:
            env, _ = make_env(n, args.mesh, tmp)
            torch.manual_seed(1)
            ac = ActorCriticRecurrent(env.num_obs, env.num_obs, env.num_actions, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128],
                                      rnn_hidden_size=args.rnn_hidden).to("cuda:0").eval()
            counter = env.ll_env._sim.buf["step_counter"]
            one = RecurrentFusedActor(ac, "cuda:0", seed=7, step_counter=counter, num_envs=n)
            assert env.shared_actor_launch(one), "lg_game_lstm_act refused the probe's actor pair"
            four = env.make_graphed_policy_step(one, steps_per_replay=2)
            if args.trace:
                for _ in range(200):
                    four()
                torch.cuda.synchronize()
                continue
            apart = RecurrentFusedActor(ac, "cuda:0", seed=7, step_counter=counter, num_envs=n)
            env._recurrent_launch = lambda *a, **k: None           # the policy stage as separate launches, for this capture only
            try:
                six = env.make_graphed_policy_step(apart, steps_per_replay=2)
            finally:
                del env._recurrent_launch
            three = env.make_graphed_policy_step(fused_high_level_actor(env), steps_per_replay=2)
            gru_four = None
            if args.gru:                               # the same step with GRU memories: lg_gru_step -> lg_game_lstm_act -> k_step -> post
                torch.manual_seed(1)
                gru_ac = ActorCriticRecurrent(env.num_obs, env.num_obs, env.num_actions, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128],
                                              rnn_type="gru", rnn_hidden_size=args.rnn_hidden).to("cuda:0").eval()
                gru_actor = RecurrentFusedActor(gru_ac, "cuda:0", seed=7, step_counter=counter, num_envs=n, gru=True)
                assert env.shared_actor_launch(gru_actor), "lg_game_lstm_act refused the probe's actor pair behind a GRU memory"
                gru_four = env.make_graphed_policy_step(gru_actor, steps_per_replay=2)
            for fn in (four, six, three) + ((gru_four,) if gru_four else ()):
                timed(fn, 100)
            r, s, f, g = [], [], [], []
            for _ in range(args.repeats):              # alternating: other work shares the machine
                r.append(timed(four, args.replays // 2) / 2)
                s.append(timed(six, args.replays // 2) / 2)
                f.append(timed(three, args.replays // 2) / 2)
                if gru_four:
                    g.append(timed(gru_four, args.replays // 2) / 2)
            gain = [y - x for x, y in zip(r, s)]
            result["envs"][str(n)] = {"recurrent_four_launch_step": spread(r), "recurrent_separate_policy_launches": spread(s),
                                      "feed_forward_three_launch_step": spread(f), "separate_minus_one_launch": spread(gain),
                                      "env_steps_per_s_recurrent_four_launch_step": n / (statistics.median(r) * 1e-6)}
            if gru_four:
                result["envs"][str(n)]["gru_four_launch_step"] = spread(g)
                result["envs"][str(n)]["gru_minus_lstm_four_launch_step"] = spread([y - x for x, y in zip(r, g)])
                print(f"{n} envs, per step: GRU four launches {statistics.median(g):.1f} us ({min(g):.1f} .. {max(g):.1f})", flush=True)
            assert torch.isfinite(env.obs_buf).all() and torch.isfinite(env.ll_env.root_states).all()
            assert all(bool(torch.isfinite(t).all()) for pair in one.hidden_states() for t in pair)
            print(f"{n} envs, per step: four launches {statistics.median(r):.1f} us ({min(r):.1f} .. {max(r):.1f}), separate policy launches "
                  f"{statistics.median(s):.1f} us ({min(s):.1f} .. {max(s):.1f}), difference {statistics.median(gain):+.2f} us ({min(gain):+.2f} .. "
                  f"{max(gain):+.2f}), feed-forward three launches {statistics.median(f):.1f} us ({min(f):.1f} .. {max(f):.1f})", flush=True)
        if args.trace:
            return
        if args.train_iterations > 0 and not args.gru:
            n = args.envs[0]
            for key, on in (("device_rollout_off", False), ("device_rollout_on", True)):
                t = train_steps_per_s(n, args.mesh, tmp, on, args.train_iterations, rnn_hidden=args.rnn_hidden)
                result["training"][key] = dict({"envs": n, "iterations": args.train_iterations}, **t)
                print(f"training, recurrent policy, {n} envs, {key}: {t['env_steps_per_s']:.0f} env-steps/s; per iteration: rollout of 24 steps "
                      f"{t['rollout_ms']['median']:.2f} ms ({t['rollout_ms']['min']:.2f} .. {t['rollout_ms']['max']:.2f}), update "
                      f"{t['update_ms']['median']:.1f} ms ({t['update_ms']['min']:.1f} .. {t['update_ms']['max']:.1f})", flush=True)
    out = args.out if args.out != DEFAULT_OUT else os.path.join(REPO, "profiles", "game_recurrent_gru_step.json" if args.gru else "game_recurrent_step.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", out)


def scripted_main(args):
    """The graphed three-launch policy step of scripted_predator_game against high_level_game's, same process, same sizes, alternating repeats."""
    result = {"device": torch.cuda.get_device_name(0), "mesh_type": args.mesh, "replays": args.replays, "repeats": args.repeats, "envs": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for n in args.envs:
            parent, _ = make_env(n, args.mesh, tmp)
            scripted, _ = make_env(n, args.mesh, tmp, scripted=True)
            step_parent = parent.make_graphed_policy_step(fused_high_level_actor(parent))
            step_scripted = scripted.make_graphed_policy_step(fused_high_level_actor(scripted))
            for fn in (step_parent, step_scripted):
                timed(fn, 200)
            a, b = [], []
            for _ in range(args.repeats):              # alternating: other work shares the machine
                a.append(timed(step_parent, args.replays))
                b.append(timed(step_scripted, args.replays))
            diff = [y - x for x, y in zip(a, b)]
            result["envs"][str(n)] = {"high_level_game_policy_step": spread(a), "scripted_predator_game_policy_step": spread(b),
                                      "scripted_minus_high_level_game": spread(diff),
                                      "env_steps_per_s_scripted_predator_game": n / (statistics.median(b) * 1e-6)}
            for env in (parent, scripted):
                assert torch.isfinite(env.obs_buf).all() and torch.isfinite(env.ll_env.root_states).all() and torch.isfinite(env.predator_pos).all()
            assert float(scripted.predator_command.abs().max()) > 0
            print(f"{n} envs, graphed three-launch policy step: high_level_game {statistics.median(a):.1f} us ({min(a):.1f} .. {max(a):.1f}), "
                  f"scripted_predator_game {statistics.median(b):.1f} us ({min(b):.1f} .. {max(b):.1f}), difference {statistics.median(diff):+.2f} us "
                  f"({min(diff):+.2f} .. {max(diff):+.2f})", flush=True)
    out = args.out if args.out != DEFAULT_OUT else os.path.join(REPO, "profiles", "pursuer_step.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", out)


def outcome_main(args):
    """The graphed three-launch policy step of both game tasks with the outcome statistics off (the parent's post kernels) and on
    (k_outcome_post), same process, same sizes, alternating repeats; the difference on - off repeat by repeat."""
    result = {"device": torch.cuda.get_device_name(0), "mesh_type": args.mesh, "replays": args.replays, "repeats": args.repeats, "envs": {}}
    names = ("high_level_game", "high_level_game_outcome", "scripted_predator_game", "scripted_predator_game_outcome")
    with tempfile.TemporaryDirectory() as tmp:
        for n in args.envs:
            envs, steps = [], []
            for scripted in (False, True):
                for on in (False, True):
                    env, _ = make_env(n, args.mesh, tmp, scripted=scripted)
                    if on:
                        env.enable_outcome_stats()           # before the capture: the graph keeps the launch the switch selected
                    envs.append(env)
                    steps.append(env.make_graphed_policy_step(fused_high_level_actor(env)))
            for fn in steps:
                timed(fn, 200)
            t = [[] for _ in steps]
            for _ in range(args.repeats):              # alternating: other work shares the machine
                for i, fn in enumerate(steps):
                    t[i].append(timed(fn, args.replays))
            row = {f"{name}_policy_step": spread(x) for name, x in zip(names, t)}
            for task, off, on in (("high_level_game", 0, 1), ("scripted_predator_game", 2, 3)):
                row[f"{task}_outcome_minus_plain"] = spread([y - x for x, y in zip(t[off], t[on])])
            for env in envs:
                assert torch.isfinite(env.obs_buf).all() and torch.isfinite(env.ll_env.root_states).all() and torch.isfinite(env.predator_pos).all()
            for i in (1, 3):
                totals = envs[i].outcome_totals()
                assert totals["episodes"] > 0 and envs[i - 1].extras == {}
                row[f"{names[i]}_totals"] = totals
            result["envs"][str(n)] = row
            print(f"{n} envs, graphed three-launch policy step: " + "; ".join(
                f"{name} {statistics.median(x):.1f} us ({min(x):.1f} .. {max(x):.1f})" for name, x in zip(names, t)), flush=True)
            for task in ("high_level_game", "scripted_predator_game"):
                d = row[f"{task}_outcome_minus_plain"]
                print(f"  {task}: statistics on - off {d['median_us']:+.2f} us ({d['min_us']:+.2f} .. {d['max_us']:+.2f})", flush=True)
    out = args.out if args.out != DEFAULT_OUT else os.path.join(REPO, "profiles", "game_outcome_step.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", out)


def timed(fn, count):
    """Mean microseconds per call of ``fn`` over ``count`` calls, device events around the whole window."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(count):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1000.0 * a.elapsed_time(b) / count


def spread(xs):
    return {"median_us": statistics.median(xs), "min_us": min(xs), "max_us": max(xs), "repeats_us": xs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="*", default=[2000, 4096])
    ap.add_argument("--replays", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--mesh", default="trimesh", help="terrain of the low-level env (the registered task: trimesh)")
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--policy-step", action="store_true", help="time the device path of the high-level actor; writes profiles/game_policy_step.json")
    ap.add_argument("--train-iterations", type=int, default=10, help="--policy-step: timed PPO iterations per setting of the runner switch (0: skip)")
    ap.add_argument("--scripted", action="store_true", help="time scripted_predator_game's graphed policy step beside high_level_game's; writes profiles/pursuer_step.json")
    ap.add_argument("--outcome", action="store_true", help="time the graphed policy step of both tasks with the outcome statistics off and on; writes profiles/game_outcome_step.json")
    ap.add_argument("--recurrent", action="store_true", help="time the recurrent policy's graphed step against separate policy launches and the feed-forward step; writes profiles/game_recurrent_step.json")
    ap.add_argument("--rnn-hidden", type=int, default=256, help="--recurrent: units per memory")
    ap.add_argument("--gru", action="store_true", help="--recurrent: also time the four-launch step with GRU memories (the key device_gru) in the same alternation, "
                    "no training; writes profiles/game_recurrent_gru_step.json")
    ap.add_argument("--trace", action="store_true", help="a short loop of graph replays only (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("game_probe needs an AMD GPU: there is nothing to time on the CPU")
    if args.recurrent:
        return recurrent_main(args)
    if args.outcome:
        return outcome_main(args)
    if args.scripted:
        return scripted_main(args)
    if args.policy_step:
        return policy_step_main(args)
    result = {"device": torch.cuda.get_device_name(0), "mesh_type": args.mesh, "replays": args.replays, "repeats": args.repeats, "envs": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for n in args.envs:
            env, policy = make_env(n, args.mesh, tmp)
            full = env.make_graphed_step(policy)
            if args.trace:
                for _ in range(200):
                    full()
                torch.cuda.synchronize()
                continue
            ll_only = graph_low_level_only(env)

            def eager():
                env.step(policy(env.obs_buf))
            for fn in (full, ll_only, eager):
                timed(fn, 200)                         # warm-up of every shape in the timed window
            a, b, c = [], [], []
            for _ in range(args.repeats):              # alternating: other work shares the machine
                a.append(timed(full, args.replays))
                b.append(timed(ll_only, args.replays))
                c.append(timed(eager, args.replays))
            over = [x - y for x, y in zip(a, b)]
            result["envs"][str(n)] = {"graphed_step": spread(a), "low_level_actor_and_step": spread(b), "eager_step": spread(c),
                                      "overhead_graphed_minus_low_level": spread(over), "env_steps_per_s_graphed": n / (statistics.median(a) * 1e-6)}
            assert torch.isfinite(env.obs_buf).all() and torch.isfinite(env.ll_env.root_states).all()
            print(f"{n} envs: graphed {statistics.median(a):.1f} us, low-level only {statistics.median(b):.1f} us, eager {statistics.median(c):.1f} us, "
                  f"overhead {statistics.median(over):.1f} us", flush=True)
    if not args.trace:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
        print("wrote", args.out)


if __name__ == "__main__":
    main()
