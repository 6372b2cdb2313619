#!/usr/bin/env python3
"""dec_high_level_game: the actor stage of a step, ``lg_dec_game_act`` (the three actors and both command clips in ONE launch) against the
four launches it replaces (``lg_policy_act`` x 3 + ``lg_dec_game_pre``) -> profiles/dec_game_act.json.

Each variant is captured into a HIP graph of ``--graph-steps`` actor stages on the device step counter; the two graphs are replayed in
alternating pairs (``--replays`` replays per timing, HIP events around them), the first ``--discard`` pairs are dropped, and the median,
minimum and maximum time per actor stage are reported per env count.  Actors are seeded random-init networks of the task's shapes
(3-512-256-128-2, 16-512-256-128-4, 235-512-256-128-12): the time does not depend on the weights.

    python tools/dec_game_probe.py [--envs 2000 4096] [--out profiles/dec_game_act.json]

``--outcome`` builds two ``DecHighLevelGame`` envs per size in one process, the outcome statistics off and on, and times their graphed
three-launch policy step (lg_dec_game_act, k_step, then k_dec_post against k_dec_outcome), alternating repeats; median and min .. max per
variant and of the difference on - off repeat by repeat -> profiles/dec_outcome_step.json.  The low-level policy is a seeded random-init
checkpoint written to a temporary directory: the kernels' cost does not depend on the weights.

    python tools/dec_game_probe.py --outcome [--envs 2000 4096] [--step-replays 2000] [--repeats 5]

``--pool`` times the actor stage with an opponent pool on the prey role (``lg_dec_pool_act``, include/legged_dec_game_pool.h) against the
plain ``lg_dec_game_act``, the way the default mode times its two variants: graphs of ``--graph-steps`` stages, replayed in alternating
rounds in one process.  Variants: the plain launch, and the pooled launch with 1, 4 and 8 members (``--members``), the 32-env blocks dealt
round-robin over the members, so that M weight sets are in flight at once -> profiles/dec_pool_act.json.

    python tools/dec_game_probe.py --pool [--envs 2000 4096] [--members 1 4 8]

``--member-outcome`` times the graphed three-launch policy step with an opponent pool of 4 members on the prey role and the outcome
statistics on, its last launch ``lg_dec_outcome_post`` (k_dec_outcome) against ``lg_dec_member_outcome_post`` (k_member_outcome, include/
legged_dec_game_member_outcome.h: the counts kept per pool member as well), by the method of ``--outcome``: both variants in one process,
alternating repeats, HIP events, median and min .. max per variant and of the difference repeat by repeat ->
profiles/dec_member_outcome_step.json.

    python tools/dec_game_probe.py --member-outcome [--envs 2000 4096] [--step-replays 2000] [--repeats 5]

``--recurrent`` times the graphed policy step with two recurrent policies (``ActorCriticRecurrent``, ``--rnn-hidden-size`` units, default 256;
the predator is the learner, so its critic memory moves too, the prey the opponent): the four-launch step (``lg_dec_lstm_step`` ->
``lg_dec_game_lstm_act`` -> k_step -> post) against the same graph with the policy stage as the eight launches of the older entry points
(``lg_lstm_step`` x 2, ``lg_lstm_actor_act`` x 2, ``lg_dec_game_pre``, ``lg_policy_act``, k_step, post) and against the feed-forward
three-launch step, by the method of ``--outcome``: one process, two-step graphs, alternating repeats, HIP events, median and min .. max per
step -> profiles/dec_recurrent_step.json.  ``--trace`` replays the four-launch graph only, for a kernel table in a run of its own:
``rocprofv3 --kernel-trace --stats -- python tools/dec_game_probe.py --recurrent --trace --envs 4096``.

    python tools/dec_game_probe.py --recurrent [--envs 2000 4096] [--step-replays 2000] [--repeats 5]

``--recurrent-pool`` times that four-launch recurrent step with the plain launches against the pooled launches of
include/legged_dec_pool_recurrent.h (``lg_dec_pool_lstm_step`` -> ``lg_dec_pool_lstm_act`` -> k_step -> post) with 1, 4 and 8 members (``--members``) of
an ``rl.RecurrentOpponentPool`` on the prey role, the 32-env blocks dealt round-robin over the members, by the same method ->
profiles/dec_recurrent_pool_step.json.

    python tools/dec_game_probe.py --recurrent-pool [--envs 2000 4096] [--members 1 4 8] [--step-replays 2000] [--repeats 5]

``--privileged`` times the graphed feed-forward policy step with the prey's privileged vector off (three launches) and on (a fourth,
``lg_dec_game_privileged_obs``, include/legged_dec_game_privileged.h, behind the post launch), by the method of ``--outcome``: one process,
alternating repeats, median [min .. max] per variant and of the difference on - off repeat by repeat -> profiles/dec_privileged_step.json.
Whether the difference is outside the spread of the repeats decides whether the writer is worth fusing into the post kernels.

    python tools/dec_game_probe.py --privileged [--envs 2000 4096] [--step-replays 2000] [--repeats 5]"""
import argparse
import json
import os
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from legged_games_gym_amd import capi  # noqa: E402
from legged_games_gym_amd.envs.a1_game.dec_high_level_game_config import DecHighLevelGameCfg  # noqa: E402
from legged_games_gym_amd.rl import ActorCritic, FusedActor  # noqa: E402

DEV = "cuda:0"
HIDDEN = [512, 256, 128]


def actor(num_obs, num_actions, seed):
    torch.manual_seed(seed)
    return FusedActor(ActorCritic(num_obs, num_obs, num_actions, actor_hidden_dims=HIDDEN, critic_hidden_dims=HIDDEN).to(DEV), DEV, seed=seed)


def params(n):
    """The clip ranges of the registered task: all the actor stage reads of ``lg_dec_game_params``."""
    r = DecHighLevelGameCfg().commands.ranges
    P = capi.lg_dec_game_params()
    P.num_envs, P.decimation, P.heading_command = n, 4, 1
    for name, key in (("cmd_lin_vel_x", "lin_vel_x"), ("cmd_lin_vel_y", "lin_vel_y"), ("predator_lin_vel_x", "predator_lin_vel_x"),
                      ("predator_lin_vel_y", "predator_lin_vel_y")):
        capi._fill(getattr(P, name), getattr(r, key))
    return P


def measure(n, graph_steps, replays, pairs, discard):
    lib = capi.load_library()
    pred, prey, ll = actor(3, 2, 5), actor(16, 4, 3), actor(235, 12, 4)
    z = lambda *s: torch.zeros(*s, device=DEV)
    prey_obs, pred_obs, ll_obs = torch.randn(n, 16, device=DEV), torch.randn(n, 3, device=DEV), torch.randn(n, 235, device=DEV)
    cy, cp, llc, act, my, mp = z(n, 4), z(n, 2), z(n, 4), z(n, 12), z(n, 4), z(n, 2)
    P = params(n)
    B = capi.dec_game_buffers({"command_prey": cy.data_ptr(), "command_pred": cp.data_ptr(), "ll_commands": llc.data_ptr()})
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    seed_prey, seed_pred = 1 + 7919, 1 + 7919 + 104729

    def one_launch():
        st = torch.cuda.current_stream().cuda_stream
        rc = capi.dec_game_act(pred.handle, prey.handle, ll.handle, P, B, pred_obs.data_ptr(), prey_obs.data_ptr(), ll_obs.data_ptr(), act.data_ptr(),
                               mp.data_ptr(), my.data_ptr(), seed_pred, seed_prey, -1, counter.data_ptr(), False, False, None, None, st)
        if rc != 0:
            raise RuntimeError("lg_dec_game_act refused the actor triple (rc -4)")

    def four_launches():
        st = torch.cuda.current_stream().cuda_stream
        for handle, obs, out, mean, seed, det in ((prey.handle, prey_obs, cy, my, seed_prey, 0), (pred.handle, pred_obs, cp, mp, seed_pred, 0)):
            if lib.lg_policy_act(handle, obs.data_ptr(), out.data_ptr(), mean.data_ptr(), n, seed, -1, counter.data_ptr(), det, st) != 0:
                raise RuntimeError(lib.lg_last_error().decode())
        capi.dec_game_pre(P, B, st)
        if lib.lg_policy_act(ll.handle, ll_obs.data_ptr(), act.data_ptr(), None, n, seed_prey, -1, counter.data_ptr(), 1, st) != 0:
            raise RuntimeError(lib.lg_last_error().decode())

    graphs = {}
    for name, fn in (("one_launch", one_launch), ("four_launches", four_launches)):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(5):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(graph_steps):
                fn()
        graphs[name] = g
    times = {k: [] for k in graphs}
    for pair in range(pairs + discard):
        for name, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(replays):
                g.replay()
            b.record()
            torch.cuda.synchronize()
            if pair >= discard:
                times[name].append(a.elapsed_time(b) * 1000.0 / (replays * graph_steps))
    return {k: {"median_us": sorted(v)[len(v) // 2], "min_us": min(v), "max_us": max(v), "repeats_us": v} for k, v in times.items()}


def alternate(graphs, replays, graph_steps, pairs, discard):
    """Replay the graphs in alternating rounds; microseconds per captured stage, the first ``discard`` rounds dropped."""
    times = {k: [] for k in graphs}
    for pair in range(pairs + discard):
        for name, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(replays):
                g.replay()
            b.record()
            torch.cuda.synchronize()
            if pair >= discard:
                times[name].append(a.elapsed_time(b) * 1000.0 / (replays * graph_steps))
    return {k: {"median_us": sorted(v)[len(v) // 2], "min_us": min(v), "max_us": max(v), "repeats_us": v} for k, v in times.items()}


def measure_pool(n, members, graph_steps, replays, pairs, discard):
    """The plain launch and the pooled launch with M members on the prey role, M in ``members``: blocks round-robin over the members."""
    pred, ll = actor(3, 2, 5), actor(235, 12, 4)
    preys = [actor(16, 4, 100 + k) for k in range(max(members))]
    z = lambda *s: torch.zeros(*s, device=DEV)
    prey_obs, pred_obs, ll_obs = torch.randn(n, 16, device=DEV), torch.randn(n, 3, device=DEV), torch.randn(n, 235, device=DEV)
    cy, cp, llc, act, my, mp = z(n, 4), z(n, 2), z(n, 4), z(n, 12), z(n, 4), z(n, 2)
    P = params(n)
    B = capi.dec_game_buffers({"command_prey": cy.data_ptr(), "command_pred": cp.data_ptr(), "ll_commands": llc.data_ptr()})
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    seed_prey, seed_pred = 1 + 7919, 1 + 7919 + 104729
    blocks = (n + capi.LG_DEC_POOL_BLOCK_ENVS - 1) // capi.LG_DEC_POOL_BLOCK_ENVS
    pools = {m: (capi.dec_pool_create([a.handle for a in preys[:m]], "prey"), (torch.arange(blocks) % m).int().to(DEV)) for m in members}

    def plain():
        st = torch.cuda.current_stream().cuda_stream
        if capi.dec_game_act(pred.handle, preys[0].handle, ll.handle, P, B, pred_obs.data_ptr(), prey_obs.data_ptr(), ll_obs.data_ptr(), act.data_ptr(),
                             mp.data_ptr(), my.data_ptr(), seed_pred, seed_prey, -1, counter.data_ptr(), False, False, None, None, st) != 0:
            raise RuntimeError("lg_dec_game_act refused the actor triple (rc -4)")

    def pooled(m):
        pool, slots = pools[m]

        def launch():
            st = torch.cuda.current_stream().cuda_stream
            if capi.dec_pool_act(pred.handle, None, ll.handle, None, None, pool, slots.data_ptr(), P, B, pred_obs.data_ptr(), prey_obs.data_ptr(),
                                 ll_obs.data_ptr(), act.data_ptr(), mp.data_ptr(), my.data_ptr(), seed_pred, seed_prey, -1, counter.data_ptr(), False, False,
                                 None, None, st) != 0:
                raise RuntimeError("lg_dec_pool_act refused the launch (rc -4)")
        return launch

    graphs = {}
    for name, fn in [("lg_dec_game_act", plain)] + [(f"lg_dec_pool_act_{m}_members", pooled(m)) for m in members]:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(5):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(graph_steps):
                fn()
        graphs[name] = g
    result = alternate(graphs, replays, graph_steps, pairs, discard)
    torch.cuda.synchronize()
    assert torch.isfinite(cy).all() and torch.isfinite(cp).all() and torch.isfinite(act).all()
    del graphs
    for pool, _ in pools.values():
        capi.dec_pool_destroy(pool)
    return result


def pool_main(args):
    out = {"device": torch.cuda.get_device_name(0), "graph_steps": args.graph_steps, "replays": args.replays, "pairs": args.pairs, "discarded_pairs": args.discard,
           "unit": "us per actor stage of one step", "pooled_role": "prey", "assignment": "block b -> member b % M",
           "envs": {str(n): measure_pool(n, args.members, args.graph_steps, args.replays, args.pairs, args.discard) for n in args.envs}}
    path = args.out if args.out != DEFAULT_OUT else os.path.join(REPO, "profiles", "dec_pool_act.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    for n, r in out["envs"].items():
        print(f"{n} envs: " + "; ".join(f"{k} {v['median_us']:.1f} us ({v['min_us']:.1f} .. {v['max_us']:.1f})" for k, v in r.items()), flush=True)
    print("wrote", path)


def make_env(n, mesh, tmp, tweak=None):
    from legged_games_gym_amd.envs import task_registry
    from legged_games_gym_amd.envs.a1_game import DecHighLevelGame, DecHighLevelGameCfg as Cfg
    from legged_games_gym_amd.utils import get_args, set_seed
    from legged_games_gym_amd.utils.helpers import class_to_dict, parse_sim_params
    a1_cfg, a1_train = task_registry.get_cfgs("a1")
    torch.manual_seed(0)
    ac = ActorCritic(a1_cfg.env.num_observations, a1_cfg.env.num_observations, a1_cfg.env.num_actions, **class_to_dict(a1_train.policy))
    ckpt = os.path.join(tmp, "model_0.pt")
    torch.save({"model_state_dict": ac.state_dict(), "optimizer_state_dict": {}, "iter": 0, "infos": None}, ckpt)
    cfg = Cfg()
    cfg.env.num_envs, cfg.env.ll_policy_path, cfg.terrain.mesh_type, cfg.seed = n, ckpt, mesh, 1
    if tweak is not None:
        tweak(cfg)
    args = get_args(["--headless", "--sim_device", DEV, "--rl_device", DEV])
    set_seed(1)
    env = DecHighLevelGame(cfg, parse_sim_params(args, {"sim": class_to_dict(cfg.sim)}), args.physics_engine, DEV, True)
    env.reset()
    return env


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


def outcome_main(args):
    """The graphed three-launch policy step with the outcome statistics off (k_dec_post, the kernel of the plain task) and on
    (k_dec_outcome): same process, same sizes, alternating repeats; the difference on - off repeat by repeat."""
    result = {"device": torch.cuda.get_device_name(0), "mesh_type": args.mesh, "replays": args.step_replays, "repeats": args.repeats,
              "unit": "us per graphed three-launch policy step", "envs": {}}
    names = ("dec_high_level_game", "dec_high_level_game_outcome")
    with tempfile.TemporaryDirectory() as tmp:
        for n in args.envs:
            envs, steps = [], []
            for on in (False, True):
                env = make_env(n, args.mesh, tmp)
                if on:
                    env.enable_outcome_stats()           # before the capture: the graph keeps the launch the switch selected
                ctr = env.ll_env._sim.buf["step_counter"]
                torch.manual_seed(1)
                fused = [FusedActor(ActorCritic(no, no, na, actor_hidden_dims=HIDDEN, critic_hidden_dims=HIDDEN).to(DEV), DEV, seed=seed, step_counter=ctr)
                         for no, na, seed in ((3, 2, 1 + 7919 + 104729), (16, 4, 1 + 7919))]
                envs.append(env)
                steps.append(env.make_graphed_policy_step(*fused))
                assert env.last_act_rc == 0
            for fn in steps:
                timed(fn, args.step_replays // 4)                # warm both graphs before the first timed window
            t = [[], []]
            for _ in range(args.repeats):
                for i, fn in enumerate(steps):
                    t[i].append(timed(fn, args.step_replays))
            row = {f"{name}_policy_step": spread(x) for name, x in zip(names, t)}
            row["outcome_minus_plain"] = spread([y - x for x, y in zip(t[0], t[1])])
            for env in envs:
                assert torch.isfinite(env.obs_buf_prey).all() and torch.isfinite(env.ll_env.root_states).all() and torch.isfinite(env.predator_pos).all()
            totals = envs[1].outcome_totals()
            assert totals["episodes"] > 0 and not any(k.startswith("outcome_") for k in envs[0].extras["episode"])
            row["dec_high_level_game_outcome_totals"] = totals
            result["envs"][str(n)] = row
            print(f"{n} envs, graphed three-launch policy step: " + "; ".join(
                f"{name} {statistics.median(x):.1f} us ({min(x):.1f} .. {max(x):.1f})" for name, x in zip(names, t)), flush=True)
            d = row["outcome_minus_plain"]
            print(f"  statistics on - off {d['median_us']:+.2f} us ({d['min_us']:+.2f} .. {d['max_us']:+.2f})", flush=True)
    out = args.out if args.out != DEFAULT_OUT else os.path.join(REPO, "profiles", "dec_outcome_step.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", out)


def privileged_main(args):
    """The graphed feed-forward policy step with the prey's privileged vector off (three launches) and on (a fourth,
    lg_dec_game_privileged_obs / k_privileged_obs, behind the post launch): same process, same sizes, alternating repeats; the difference
    on - off repeat by repeat, to be read against the spread of the repeats."""
    result = {"device": torch.cuda.get_device_name(0), "mesh_type": args.mesh, "replays": args.step_replays, "repeats": args.repeats,
              "unit": "us per graphed policy step (three launches; four with the prey's privileged vector)", "envs": {}}
    names = ("privileged_off", "privileged_prey")

    def prey_vector(cfg):
        cfg.env.num_privileged_obs_prey = 22
    with tempfile.TemporaryDirectory() as tmp:
        for n in args.envs:
            envs, steps = [], []
            for on in (False, True):
                env = make_env(n, args.mesh, tmp, prey_vector if on else None)
                ctr = env.ll_env._sim.buf["step_counter"]
                torch.manual_seed(1)
                fused = [FusedActor(ActorCritic(no, no, na, actor_hidden_dims=HIDDEN, critic_hidden_dims=HIDDEN).to(DEV), DEV, seed=seed, step_counter=ctr)
                         for no, na, seed in ((3, 2, 1 + 7919 + 104729), (16, 4, 1 + 7919))]
                envs.append(env)
                steps.append(env.make_graphed_policy_step(*fused))
                assert env.last_act_rc == 0
            for fn in steps:
                timed(fn, args.step_replays // 4)                # warm both graphs before the first timed window
            t = [[], []]
            for _ in range(args.repeats):
                for i, fn in enumerate(steps):
                    t[i].append(timed(fn, args.step_replays))
            row = {f"{name}_policy_step": spread(x) for name, x in zip(names, t)}
            row["on_minus_off"] = spread([y - x for x, y in zip(t[0], t[1])])
            for env in envs:
                assert torch.isfinite(env.obs_buf_prey).all() and torch.isfinite(env.ll_env.root_states).all() and torch.isfinite(env.predator_pos).all()
            assert envs[0].privileged_obs_buf_prey is None and torch.equal(envs[1].privileged_obs_buf_prey[:, :16], envs[1].obs_buf_prey)
            result["envs"][str(n)] = row
            print(f"{n} envs, graphed policy step: " + "; ".join(
                f"{name} {statistics.median(x):.1f} us [{min(x):.1f} .. {max(x):.1f}]" for name, x in zip(names, t)), flush=True)
            d = row["on_minus_off"]
            print(f"  privileged on - off {d['median_us']:+.2f} us [{d['min_us']:+.2f} .. {d['max_us']:+.2f}]", flush=True)
    out = args.out if args.out != DEFAULT_OUT else os.path.join(REPO, "profiles", "dec_privileged_step.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", out)


def member_outcome_main(args):
    """The graphed three-launch policy step against a 4-member prey pool with the outcome statistics on, the last launch k_dec_outcome (pooled
    counts) against k_member_outcome (the counts per pool member as well): same process, same sizes, alternating repeats; the difference
    member - pooled repeat by repeat."""
    from legged_games_gym_amd.rl import OpponentPool
    members = 4
    result = {"device": torch.cuda.get_device_name(0), "mesh_type": args.mesh, "replays": args.step_replays, "repeats": args.repeats, "pool_role": "prey",
              "pool_members": members, "unit": "us per graphed three-launch policy step", "envs": {}}
    names = ("lg_dec_outcome_post", "lg_dec_member_outcome_post")
    with tempfile.TemporaryDirectory() as tmp:
        for n in args.envs:
            envs, steps, pools = [], [], []
            for per_member in (False, True):
                env = make_env(n, args.mesh, tmp)
                env.enable_outcome_stats()
                ctr = env.ll_env._sim.buf["step_counter"]
                torch.manual_seed(1)
                pred, prey = [FusedActor(ActorCritic(no, no, na, actor_hidden_dims=HIDDEN, critic_hidden_dims=HIDDEN).to(DEV), DEV, seed=seed, step_counter=ctr)
                              for no, na, seed in ((3, 2, 1 + 7919 + 104729), (16, 4, 1 + 7919))]
                pool = OpponentPool(prey, lambda: ActorCritic(16, 16, 4, actor_hidden_dims=HIDDEN, critic_hidden_dims=HIDDEN).to(DEV), members - 1, "prey", seed=1, num_envs=n)
                for k in range(members - 1):
                    torch.manual_seed(10 + k)
                    pool.push(ActorCritic(16, 16, 4, actor_hidden_dims=HIDDEN, critic_hidden_dims=HIDDEN).to(DEV).state_dict(), pushed_at=k)
                pool.set_slots(torch.arange(pool.slot_table(n).shape[0]) % members)          # the blocks dealt round-robin: all four members in flight
                if per_member:
                    env.enable_member_outcomes(pool)     # before the capture: the graph keeps the launch the switch selected
                envs.append(env); pools.append(pool)
                steps.append(env.make_graphed_policy_step(pred, pool))
                assert env.last_act_rc == 0
            for fn in steps:
                timed(fn, args.step_replays // 4)                # warm both graphs before the first timed window
            t = [[], []]
            for _ in range(args.repeats):
                for i, fn in enumerate(steps):
                    t[i].append(timed(fn, args.step_replays))
            row = {f"{name}_policy_step": spread(x) for name, x in zip(names, t)}
            row["member_minus_pooled"] = spread([y - x for x, y in zip(t[0], t[1])])
            for env in envs:
                assert torch.isfinite(env.obs_buf_prey).all() and torch.isfinite(env.ll_env.root_states).all() and torch.isfinite(env.predator_pos).all()
            totals, rows = envs[1].outcome_totals(), pools[1].member_totals_host()
            assert totals["episodes"] > 0 and {k: sum(r[k] for r in rows) for k in totals} == totals and not pools[0].member_totals.any()
            row["outcome_totals"], row["member_totals"] = totals, rows
            result["envs"][str(n)] = row
            print(f"{n} envs, graphed three-launch policy step, last launch: " + "; ".join(
                f"{name} {statistics.median(x):.1f} us ({min(x):.1f} .. {max(x):.1f})" for name, x in zip(names, t)), flush=True)
            d = row["member_minus_pooled"]
            print(f"  per member - pooled {d['median_us']:+.2f} us ({d['min_us']:+.2f} .. {d['max_us']:+.2f})", flush=True)
    out = args.out if args.out != DEFAULT_OUT else os.path.join(REPO, "profiles", "dec_member_outcome_step.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", out)


def recurrent_pair(env, units, wide=False, gru=False, shared_gru=False):
    """Two ``RecurrentFusedActor`` s of the task's default actor widths on the env's device step counter (seeded random-init policies: the
    time does not depend on the weights).  ``wide``: the handles of liblegged_lstm_wide.so where ``units`` is above 256.  ``gru``: GRU memories on the handles of liblegged_gru.so;
    ``shared_gru``: such a pair on the shared launches (the key dec_gru_shared)."""
    from legged_games_gym_amd.rl import ActorCriticRecurrent
    from legged_games_gym_amd.rl.recurrent_actor import RecurrentFusedActor
    ctr = env.ll_env._sim.buf["step_counter"]
    torch.manual_seed(1)
    return [RecurrentFusedActor(ActorCriticRecurrent(no, no, na, actor_hidden_dims=HIDDEN, critic_hidden_dims=HIDDEN, rnn_hidden_size=units,
                                                     rnn_type="gru" if gru else "lstm").to(DEV), DEV,
                                seed=seed, step_counter=ctr, num_envs=env.num_envs, wide=wide, gru=gru, shared_gru=shared_gru) for no, na, seed in ((3, 2, 1 + 7919 + 104729), (16, 4, 1 + 7919))]


def separate_recurrent_step(env, pred, prey):
    """The eight-launch step of the older entry points on the actors' own slots: ``lg_lstm_step`` with the learner's (predator's) actor and
    critic memory, ``lg_lstm_step`` with the opponent's (prey's) actor memory, ``lg_lstm_actor_act`` x 2, ``lg_dec_game_pre``, the low-level
    ``lg_policy_act``, k_step, the post kernel.  No copy kernels: the opponent's critic memory rests in both of its slots."""
    from legged_games_gym_amd.rl.recurrent_actor import lstm_step
    n, lib = env.num_envs, pred.cell_lib

    def device_step():
        stream = torch.cuda.current_stream().cuda_stream
        h = []
        for fused, obs, with_c in ((pred, env.obs_buf_pred, True), (prey, env.obs_buf_prey, False)):
            f = fused._flip
            lstm_step(lib, fused.lstm_a, fused.lstm_c if with_c else None, obs, obs if with_c else None, env.reset_buf, fused.state_a[f], fused.state_a[1 - f],
                      fused.state_c[f], fused.state_c[1 - f], n, stream)
            h.append(fused.state_a[1 - f][0])
            fused._flip = 1 - f
        (cp, _), (cy, _) = pred.fused.act_with_mean(h[0]), prey.fused.act_with_mean(h[1])
        B = env._bind(cp, cy, env.obs_buf_pred, env.obs_buf_prey)
        capi.dec_game_pre(env._P, B, stream)
        ll_actions = env.ll_policy(env.ll_env.obs_buf)
        env.ll_env._sim.step(ll_actions, -1)
        env._post(B, -1, stream)
    return device_step


def recurrent_main(args):
    """Two-step graphs of the policy step: recurrent in four launches, recurrent with the policy stage as separate launches, feed-forward in
    three launches; same process, same sizes, alternating repeats; microseconds per STEP."""
    S = 2
    names = ("recurrent_four_launch_step", "recurrent_separate_policy_launches", "feed_forward_three_launch_step")
    result = {"device": torch.cuda.get_device_name(0), "mesh_type": args.mesh, "replays": args.step_replays, "repeats": args.repeats,
              "rnn_hidden_size": args.rnn_hidden_size, "steps_per_replay": S, "learner": "pred (its critic memory moves)", "unit": "us per policy step", "envs": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for n in args.envs:
            envs, steps, actors = [], [], []                     # (a graph reads its actors' weights and memories where they are: all kept until the size is done)
            env = make_env(n, args.mesh, tmp)
            pred, prey = recurrent_pair(env, args.rnn_hidden_size)
            actors.append((pred, prey))
            if env.shared_actor_launch(pred, prey) is not True:          # raises the LDS limits outside the capture
                raise RuntimeError("lg_dec_game_lstm_act refused the actors")
            steps.append(env.make_graphed_policy_step(pred, prey, steps_per_replay=S, with_critic_memory=("pred",)))
            assert env.last_act_rc == 0
            envs.append(env)
            if args.trace:
                for _ in range(args.step_replays // S):
                    steps[0]()
                torch.cuda.synchronize()
                assert torch.isfinite(env.obs_buf_prey).all()
                print(f"{n} envs: {args.step_replays} steps of the four-launch graph replayed")
                continue
            env = make_env(n, args.mesh, tmp)
            pred, prey = recurrent_pair(env, args.rnn_hidden_size)
            actors.append((pred, prey))
            env._policy_step_graph, replay = env._capture(separate_recurrent_step(env, pred, prey), 3, S, env._step_result)
            steps.append(replay)
            envs.append(env)
            env = make_env(n, args.mesh, tmp)
            ctr = env.ll_env._sim.buf["step_counter"]
            torch.manual_seed(1)
            fused = [FusedActor(ActorCritic(no, no, na, actor_hidden_dims=HIDDEN, critic_hidden_dims=HIDDEN).to(DEV), DEV, seed=seed, step_counter=ctr)
                     for no, na, seed in ((3, 2, 1 + 7919 + 104729), (16, 4, 1 + 7919))]
            actors.append(fused)
            steps.append(env.make_graphed_policy_step(*fused, steps_per_replay=S))
            assert env.last_act_rc == 0
            envs.append(env)
            for fn in steps:
                timed(fn, args.step_replays // (4 * S))          # warm every graph before the first timed window
            t = [[] for _ in steps]
            for _ in range(args.repeats):
                for i, fn in enumerate(steps):
                    t[i].append(timed(fn, args.step_replays // S) / S)
            row = {name: spread(x) for name, x in zip(names, t)}
            row["separate_minus_four_launch"] = spread([y - x for x, y in zip(t[0], t[1])])
            row["four_launch_minus_feed_forward"] = spread([x - z for x, z in zip(t[0], t[2])])
            row["env_steps_per_s_recurrent_four_launch_step"] = n / (statistics.median(t[0]) * 1e-6)
            for env in envs:
                assert torch.isfinite(env.obs_buf_prey).all() and torch.isfinite(env.ll_env.root_states).all() and torch.isfinite(env.predator_pos).all()
            result["envs"][str(n)] = row
            print(f"{n} envs, per step of a two-step graph: " + "; ".join(f"{name} {statistics.median(x):.1f} us ({min(x):.1f} .. {max(x):.1f})" for name, x in zip(names, t)),
                  flush=True)
            d = row["separate_minus_four_launch"]
            print(f"  separate - four launches {d['median_us']:+.2f} us ({d['min_us']:+.2f} .. {d['max_us']:+.2f})", flush=True)
            torch.cuda.synchronize()
            del steps, envs, actors
    if args.trace:
        return
    out = args.out if args.out != DEFAULT_OUT else os.path.join(REPO, "profiles", "dec_recurrent_step.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", out)


def wide_main(args):
    """Two-step graphs of the policy step with two recurrent policies: ``--wide-hidden-size`` units (default 512) with the key ``wide_memory`` --
    the six-launch policy stage ``lg_lstm_wide_step`` x 2, ``lg_lstm_wide_actor_act`` x 2, ``lg_dec_game_pre``, ``lg_policy_act`` -- against the
    four-launch step at 256 units; same process, same sizes, alternating repeats; microseconds per STEP."""
    S = 2
    names = ("wide_separate_launch_step", "recurrent_four_launch_step_256_units")
    result = {"device": torch.cuda.get_device_name(0), "mesh_type": args.mesh, "replays": args.step_replays, "repeats": args.repeats,
              "wide_hidden_size": args.wide_hidden_size, "steps_per_replay": S, "learner": "pred (its critic memory moves)", "unit": "us per policy step", "envs": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for n in args.envs:
            envs, steps, actors = [], [], []
            for units, wide in ((args.wide_hidden_size, True), (256, False)):
                env = make_env(n, args.mesh, tmp)
                pred, prey = recurrent_pair(env, units, wide=wide)
                actors.append((pred, prey))
                shared = env.shared_actor_launch(pred, prey)
                if shared is not (not wide):                     # the wide pair takes the separate launches, the 256-unit pair the shared ones
                    raise RuntimeError(f"shared_actor_launch returned {shared} for {units} units")
                steps.append(env.make_graphed_policy_step(pred, prey, steps_per_replay=S, with_critic_memory=("pred",)))
                assert env.last_act_rc == (-4 if wide else 0)
                envs.append(env)
            for fn in steps:
                timed(fn, args.step_replays // (4 * S))          # warm every graph before the first timed window
            t = [[] for _ in steps]
            for _ in range(args.repeats):
                for i, fn in enumerate(steps):
                    t[i].append(timed(fn, args.step_replays // S) / S)
            row = {name: spread(x) for name, x in zip(names, t)}
            row["wide_minus_four_launch"] = spread([x - y for x, y in zip(t[0], t[1])])
            for env in envs:
                assert torch.isfinite(env.obs_buf_prey).all() and torch.isfinite(env.ll_env.root_states).all() and torch.isfinite(env.predator_pos).all()
            result["envs"][str(n)] = row
            print(f"{n} envs, per step of a two-step graph: " + "; ".join(f"{name} {statistics.median(x):.1f} us ({min(x):.1f} .. {max(x):.1f})" for name, x in zip(names, t)),
                  flush=True)
            torch.cuda.synchronize()
            del steps, envs, actors
    out = args.out if args.out != DEFAULT_OUT else os.path.join(REPO, "profiles", "dec_recurrent_wide_step.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", out)


def gru_main(args):
    """Two-step graphs of the policy step with two recurrent policies of ``--rnn-hidden-size`` units: GRU memories with the key ``device_gru`` --
    the six-launch policy stage ``lg_gru_step`` x 2, ``lg_lstm_actor_act`` x 2, ``lg_dec_game_pre``, ``lg_policy_act`` -- against the four-launch
    step of two LSTM policies; same process, same sizes, alternating repeats; microseconds per STEP."""
    S = 2
    names = ("gru_separate_launch_step", "lstm_four_launch_step")
    result = {"device": torch.cuda.get_device_name(0), "mesh_type": args.mesh, "replays": args.step_replays, "repeats": args.repeats,
              "rnn_hidden_size": args.rnn_hidden_size, "steps_per_replay": S, "learner": "pred (its critic memory moves)", "unit": "us per policy step", "envs": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for n in args.envs:
            envs, steps, actors = [], [], []
            for gru in (True, False):
                env = make_env(n, args.mesh, tmp)
                pred, prey = recurrent_pair(env, args.rnn_hidden_size, gru=gru)
                actors.append((pred, prey))
                shared = env.shared_actor_launch(pred, prey)
                if shared is not (not gru):                      # the GRU pair takes the separate launches, the LSTM pair the shared ones
                    raise RuntimeError(f"shared_actor_launch returned {shared} for gru={gru}")
                steps.append(env.make_graphed_policy_step(pred, prey, steps_per_replay=S, with_critic_memory=("pred",)))
                assert env.last_act_rc == (-4 if gru else 0)
                envs.append(env)
            for fn in steps:
                timed(fn, args.step_replays // (4 * S))          # warm every graph before the first timed window
            t = [[] for _ in steps]
            for _ in range(args.repeats):
                for i, fn in enumerate(steps):
                    t[i].append(timed(fn, args.step_replays // S) / S)
            row = {name: spread(x) for name, x in zip(names, t)}
            row["gru_minus_lstm"] = spread([x - y for x, y in zip(t[0], t[1])])
            for env in envs:
                assert torch.isfinite(env.obs_buf_prey).all() and torch.isfinite(env.ll_env.root_states).all() and torch.isfinite(env.predator_pos).all()
            result["envs"][str(n)] = row
            print(f"{n} envs, per step of a two-step graph: " + "; ".join(f"{name} {statistics.median(x):.1f} us ({min(x):.1f} .. {max(x):.1f})" for name, x in zip(names, t)),
                  flush=True)
            torch.cuda.synchronize()
            del steps, envs, actors
    out = args.out if args.out != DEFAULT_OUT else os.path.join(REPO, "profiles", "dec_recurrent_gru_step.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", out)


def gru_shared_main(args):
    """``gru_main`` with a third variant in front: the GRU pair with the key ``dec_gru_shared`` on top of ``device_gru`` -- the two-launch policy
    stage ``lg_dec_gru_step`` -> ``lg_dec_game_lstm_act`` -- against the six-launch policy stage of ``device_gru`` alone (the yardstick: that path
    is the one ``gru_main`` times) and the four-launch step of two LSTM policies (context); same process, same sizes, alternating repeats;
    microseconds per STEP."""
    S = 2
    names = ("gru_shared_step", "gru_separate_launch_step", "lstm_four_launch_step")
    variants = ((True, True), (True, False), (False, False))         # (gru, shared_gru)
    result = {"device": torch.cuda.get_device_name(0), "mesh_type": args.mesh, "replays": args.step_replays, "repeats": args.repeats,
              "rnn_hidden_size": args.rnn_hidden_size, "steps_per_replay": S, "learner": "pred (its critic memory moves)", "unit": "us per policy step", "envs": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for n in args.envs:
            envs, steps, actors = [], [], []
            for gru, shared_gru in variants:
                env = make_env(n, args.mesh, tmp)
                pred, prey = recurrent_pair(env, args.rnn_hidden_size, gru=gru, shared_gru=shared_gru)
                actors.append((pred, prey))
                shared = env.shared_actor_launch(pred, prey)
                if shared is not (shared_gru or not gru):            # only the GRU pair without the key takes the separate launches
                    raise RuntimeError(f"shared_actor_launch returned {shared} for gru={gru}, shared_gru={shared_gru}")
                steps.append(env.make_graphed_policy_step(pred, prey, steps_per_replay=S, with_critic_memory=("pred",)))
                assert env.last_act_rc == (0 if shared else -4)
                envs.append(env)
            for fn in steps:
                timed(fn, args.step_replays // (4 * S))          # warm every graph before the first timed window
            t = [[] for _ in steps]
            for _ in range(args.repeats):
                for i, fn in enumerate(steps):
                    t[i].append(timed(fn, args.step_replays // S) / S)
            row = {name: spread(x) for name, x in zip(names, t)}
            row["shared_minus_separate"] = spread([x - y for x, y in zip(t[0], t[1])])
            row["shared_minus_lstm"] = spread([x - y for x, y in zip(t[0], t[2])])
            for env in envs:
                assert torch.isfinite(env.obs_buf_prey).all() and torch.isfinite(env.ll_env.root_states).all() and torch.isfinite(env.predator_pos).all()
            result["envs"][str(n)] = row
            print(f"{n} envs, per step of a two-step graph: " + "; ".join(f"{name} {statistics.median(x):.1f} us ({min(x):.1f} .. {max(x):.1f})" for name, x in zip(names, t)),
                  flush=True)
            torch.cuda.synchronize()
            del steps, envs, actors
    out = args.out if args.out != DEFAULT_OUT else os.path.join(REPO, "profiles", "dec_recurrent_gru_shared_step.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", out)


def recurrent_pool_main(args):
    """Two-step graphs of the four-launch recurrent policy step: the plain launches (``lg_dec_lstm_step`` -> ``lg_dec_game_lstm_act``) against the
    pooled launches (``lg_dec_pool_lstm_step`` -> ``lg_dec_pool_lstm_act``) with --members members on the prey role, the blocks dealt round-robin;
    same process, same sizes, alternating repeats; microseconds per STEP."""
    from legged_games_gym_amd.rl import ActorCriticRecurrent, RecurrentOpponentPool
    S, units = 2, args.rnn_hidden_size
    names = ["plain_four_launch_step"] + [f"pooled_{m}_members" for m in args.members]
    result = {"device": torch.cuda.get_device_name(0), "mesh_type": args.mesh, "replays": args.step_replays, "repeats": args.repeats, "rnn_hidden_size": units,
              "steps_per_replay": S, "pool_role": "prey", "learner": "pred (its critic memory moves)", "unit": "us per policy step", "envs": {}}
    module = lambda: ActorCriticRecurrent(16, 16, 4, actor_hidden_dims=HIDDEN, critic_hidden_dims=HIDDEN, rnn_hidden_size=units).to(DEV)
    with tempfile.TemporaryDirectory() as tmp:
        for n in args.envs:
            envs, steps, actors = [], [], []                     # (a graph reads its actors' weights and memories where they are: all kept until the size is done)
            for members in [0] + list(args.members):
                env = make_env(n, args.mesh, tmp)
                pred, prey = recurrent_pair(env, units)
                opponent = prey
                if members:
                    opponent = RecurrentOpponentPool(prey, module, max(1, members - 1), "prey", seed=1, num_envs=n)
                    for k in range(members - 1):
                        torch.manual_seed(10 + k)
                        opponent.push(module().state_dict(), pushed_at=k)
                    opponent.set_slots(torch.arange(opponent.slot_table(n).shape[0]) % members)      # round-robin: all members in flight
                if env.shared_actor_launch(pred, opponent) is not True:      # raises the LDS limits outside the capture
                    raise RuntimeError("the recurrent actor launch refused the actors")
                steps.append(env.make_graphed_policy_step(pred, opponent, steps_per_replay=S, with_critic_memory=("pred",)))
                assert env.last_act_rc == 0
                envs.append(env); actors.append((pred, opponent))
            for fn in steps:
                timed(fn, args.step_replays // (4 * S))          # warm every graph before the first timed window
            t = [[] for _ in steps]
            for _ in range(args.repeats):
                for i, fn in enumerate(steps):
                    t[i].append(timed(fn, args.step_replays // S) / S)
            row = {name: spread(x) for name, x in zip(names, t)}
            for name, x in zip(names[1:], t[1:]):
                row[f"{name}_minus_plain"] = spread([y - z for z, y in zip(t[0], x)])
            for env in envs:
                assert torch.isfinite(env.obs_buf_prey).all() and torch.isfinite(env.ll_env.root_states).all() and torch.isfinite(env.predator_pos).all()
            result["envs"][str(n)] = row
            print(f"{n} envs, per step of a two-step graph: " + "; ".join(f"{name} {statistics.median(x):.1f} us ({min(x):.1f} .. {max(x):.1f})" for name, x in zip(names, t)),
                  flush=True)
            torch.cuda.synchronize()
            del steps, envs, actors
    out = args.out if args.out != DEFAULT_OUT else os.path.join(REPO, "profiles", "dec_recurrent_pool_step.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", out)


DEFAULT_OUT = os.path.join(REPO, "profiles", "dec_game_act.json")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--envs", type=int, nargs="+", default=[2000, 4096])
    ap.add_argument("--graph-steps", type=int, default=50)
    ap.add_argument("--replays", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--discard", type=int, default=2)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--outcome", action="store_true", help="time the graphed policy step with the outcome statistics off and on; writes profiles/dec_outcome_step.json")
    ap.add_argument("--step-replays", type=int, default=2000, help="--outcome: replays of the captured step per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="--outcome: timed windows per variant, alternating")
    ap.add_argument("--mesh", default="plane", help="--outcome: terrain of the low-level env (the registered task: plane)")
    ap.add_argument("--pool", action="store_true", help="time lg_dec_pool_act with --members members on the prey role against lg_dec_game_act; writes profiles/dec_pool_act.json")
    ap.add_argument("--members", type=int, nargs="+", default=[1, 4, 8], help="--pool: pool sizes to time")
    ap.add_argument("--member-outcome", action="store_true", help="time the graphed policy step against a 4-member prey pool with lg_dec_outcome_post and with "
                    "lg_dec_member_outcome_post as the last launch; writes profiles/dec_member_outcome_step.json")
    ap.add_argument("--recurrent", action="store_true", help="time the graphed policy step with two recurrent policies in four launches, with the policy stage as "
                    "separate launches, and the feed-forward three-launch step; writes profiles/dec_recurrent_step.json")
    ap.add_argument("--rnn-hidden-size", type=int, default=256, help="--recurrent: units of every memory")
    ap.add_argument("--wide", action="store_true", help="time the graphed policy step with two wide recurrent policies (the key wide_memory: separate launches "
                    "of liblegged_lstm_wide.so) against the four-launch step at 256 units; writes profiles/dec_recurrent_wide_step.json")
    ap.add_argument("--gru", action="store_true", help="time the graphed policy step with two GRU policies (the key device_gru: separate launches, "
                    "liblegged_gru.so) against the four-launch step of two LSTM policies at --rnn-hidden-size units; writes profiles/dec_recurrent_gru_step.json")
    ap.add_argument("--gru-shared", action="store_true", help="--gru with the GRU pair on the shared launches as well (the key dec_gru_shared: lg_dec_gru_step -> "
                    "lg_dec_game_lstm_act), the three variants alternating in one process; writes profiles/dec_recurrent_gru_shared_step.json")
    ap.add_argument("--wide-hidden-size", type=int, default=512, help="--wide: units of every memory of the wide pair")
    ap.add_argument("--trace", action="store_true", help="--recurrent: replay the four-launch graph only and write nothing (for a rocprofv3 kernel table)")
    ap.add_argument("--recurrent-pool", action="store_true", help="time the four-launch recurrent policy step with the plain launches against the pooled launches "
                    "with --members members on the prey role; writes profiles/dec_recurrent_pool_step.json")
    ap.add_argument("--privileged", action="store_true", help="time the graphed policy step with the prey's privileged vector off and on (one more launch, "
                    "lg_dec_game_privileged_obs); writes profiles/dec_privileged_step.json")
    args = ap.parse_args()
    if args.privileged:
        return privileged_main(args)
    if args.wide:
        return wide_main(args)
    if args.gru_shared:
        return gru_shared_main(args)
    if args.gru:
        return gru_main(args)
    if args.recurrent_pool:
        return recurrent_pool_main(args)
    if args.recurrent:
        return recurrent_main(args)
    if args.outcome:
        return outcome_main(args)
    if args.member_outcome:
        return member_outcome_main(args)
    if args.pool:
        return pool_main(args)
    out = {"device": torch.cuda.get_device_name(0), "graph_steps": args.graph_steps, "replays": args.replays, "pairs": args.pairs, "discarded_pairs": args.discard,
           "unit": "us per actor stage of one step", "role_order": "low-level, prey, predator (the other orders are not timed)",
           "envs": {str(n): measure(n, args.graph_steps, args.replays, args.pairs, args.discard) for n in args.envs}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({n: {k: round(v["median_us"], 2) for k, v in r.items()} for n, r in out["envs"].items()}))


if __name__ == "__main__":
    main()
