#!/usr/bin/env python3
"""Cost of the game layer around the low-level step (GPU only).

Times, with device events around >= 2000 replays after warm-up, alternating in one process, at the registered 2000 envs and at 4096:
  (a) the graphed high-level step (``HighLevelGame.make_graphed_step``) with a random-init 19-512-256-128-6 policy:
      high-level actor, k_game_pre, low-level actor, k_step, k_game_post;
  (b) the same graph without the two game kernels and without the high-level actor (low-level actor + k_step: one `a1` policy step);
  (c) the eager ``step``.
Writes profiles/game_step.json (or --out): the three times per repeat, their spread over the repeats, the overhead (a) - (b) and the
env-steps/s of (a).  ``--trace`` runs a short replay loop only, for ``rocprofv3 --kernel-trace --stats -- python tools/game_probe.py --trace``.

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


def make_env(n, mesh, tmp):
    from legged_games_gym_amd.envs import task_registry
    from legged_games_gym_amd.envs.a1_game import HighLevelGame, HighLevelGameFlatCfg
    from legged_games_gym_amd.rl import ActorCritic
    from legged_games_gym_amd.utils import get_args, set_seed
    from legged_games_gym_amd.utils.helpers import class_to_dict, parse_sim_params
    a1_cfg, a1_train = task_registry.get_cfgs("a1")
    torch.manual_seed(0)
    ac = ActorCritic(a1_cfg.env.num_observations, a1_cfg.env.num_observations, a1_cfg.env.num_actions, **class_to_dict(a1_train.policy))
    ckpt = os.path.join(tmp, "model_0.pt")
    torch.save({"model_state_dict": ac.state_dict(), "optimizer_state_dict": {}, "iter": 0, "infos": None}, ckpt)
    cfg = HighLevelGameFlatCfg()
    cfg.env.num_envs, cfg.env.ll_policy_path, cfg.terrain.mesh_type, cfg.seed = n, ckpt, mesh, 1
    args = get_args(["--headless", "--sim_device", "cuda:0", "--rl_device", "cuda:0"])
    set_seed(1)
    env = HighLevelGame(cfg, parse_sim_params(args, {"sim": class_to_dict(cfg.sim)}), args.physics_engine, "cuda:0", True)
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "game_step.json"))
    ap.add_argument("--trace", action="store_true", help="a short loop of graph replays only (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("game_probe needs an AMD GPU: there is nothing to time on the CPU")
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
