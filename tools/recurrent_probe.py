"""The policy stage of a recurrent policy on the device path against the same stage in torch -> profiles/recurrent_step.json.

Method of tools/dec_game_probe.py: HIP events, each variant a graph of ``--graph-steps`` stages, replayed in alternating repeats, median
[min .. max] per variant.  Variants, at 2000 and 4096 envs, 48 inputs, 64 and 256 units, the flat task's 128-64-32 actor and critic:

  device   lg_lstm_step (both memories) + lg_lstm_actor_act            (rl.RecurrentFusedActor.act_with_mean)
  torch    ActorCriticRecurrent.act + evaluate under inference_mode    (what the generic loop runs per step)
  cell     lg_lstm_step alone: the kernel's time against its 2 x 2 N (I + H) 4H FLOP, i.e. its share of the f32-MFMA peak

The ``torch`` stage is captured like the others; ``Memory.forward`` leaves its state in a new tensor every step, so the stage copies
the state back into buffers that live as long as the graph and starts every step from them (four copies the generic loop does not make).

``--train`` adds the training throughput of anymal_c_flat with the recurrent policy, ``fused_rollout`` on and off, in one process.
Run on the GPU: ``python tools/recurrent_probe.py [--train]``.

The kernel's own time, independent of the event timing above, comes from a profiler run of its own:
``rocprofv3 --kernel-trace --stats -d <dir> -- python tools/recurrent_probe.py --cell-only`` launches ``lg_lstm_step`` (both memories,
4096 envs, 48 inputs, 256 units) 200 times eagerly and nothing else; the ``k_lstm_cell`` row of the kernel statistics against
``flop`` / 155 TF is its share of the f32-MFMA peak.

``--wide`` measures the wide library instead (include/legged_recurrent_wide.h, the runner key ``wide_memory``) -> profiles/recurrent_wide_step.json:
the same three variants at 512 units (``lg_lstm_wide_step`` + ``lg_lstm_wide_actor_act`` against torch, the cell against its FLOP count), and at
256 units ``lg_lstm_wide_step`` against ``lg_lstm_step`` on the same memories, all in one process.

``--gru`` measures the GRU library instead (include/legged_recurrent_gru.h, the runner key ``device_gru``) -> profiles/recurrent_gru_step.json:
the three variants with ``rnn_type='gru'`` (``lg_gru_step`` + ``lg_lstm_actor_act`` against torch, the cell against its 3/4 FLOP count) and,
in the same alternation, ``lstm``: the device stage of the LSTM policy of the same width."""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, REPO)
DEV = "cuda:0"
PEAK_F32_MFMA = 155e12          # measured f32-MFMA rate of the MI355X, FLOP/s


def capture(fn, stages):
    """A graph of ``stages`` calls of ``fn``, or None where the capture is refused (the stage is then timed as eager launches)."""
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    try:
        with torch.cuda.stream(side):
            for _ in range(2):
                fn()                                          # warm-up on the capture stream
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                for _ in range(stages):
                    fn()
        torch.cuda.current_stream().wait_stream(side)
        return g
    except Exception as exc:
        print(f"  capture refused ({type(exc).__name__}: {exc}); eager launches", flush=True)
        torch.cuda.synchronize()
        return None


def alternate(variants, stages, replays, pairs, discard):
    times = {k: [] for k in variants}
    for pair in range(pairs + discard):
        for name, (g, fn) in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(replays):
                if g is not None:
                    g.replay()
                else:
                    for _ in range(stages):
                        fn()
            b.record()
            torch.cuda.synchronize()
            if pair >= discard:
                times[name].append(a.elapsed_time(b) * 1000.0 / (replays * stages))
    return {k: {"median_us": sorted(v)[len(v) // 2], "min_us": min(v), "max_us": max(v), "repeats_us": v, "captured": variants[k][0] is not None}
            for k, v in times.items()}


def measure(n, hidden, args, wide=False, gru=False):
    from legged_games_gym_amd.rl import ActorCriticRecurrent
    from legged_games_gym_amd.rl.recurrent_actor import RecurrentFusedActor, gru_step, lstm_step
    torch.manual_seed(1)
    ac = ActorCriticRecurrent(48, 48, 12, actor_hidden_dims=[128, 64, 32], critic_hidden_dims=[128, 64, 32], rnn_hidden_size=hidden,
                              rnn_type="gru" if gru else "lstm").to(DEV)
    rfa = RecurrentFusedActor(ac, DEV, seed=3, num_envs=n, wide=wide, gru=gru)
    obs = torch.rand(n, 48, device=DEV) * 6.0 - 3.0
    reset = (torch.rand(n, device=DEV) < 0.02)

    def device():
        rfa.act_with_mean(obs, obs, reset=reset)

    def gru_cell():
        f = rfa._flip
        gru_step(rfa.cell_lib, rfa.lstm_a, rfa.lstm_c, obs, obs, reset, rfa.state_a[f][0], rfa.state_a[1 - f][0], rfa.state_c[f][0], rfa.state_c[1 - f][0], n,
                 torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
        rfa._flip = 1 - f

    def cell():
        if gru:
            return gru_cell()
        f = rfa._flip
        lstm_step(rfa.cell_lib, rfa.lstm_a, rfa.lstm_c, obs, obs, reset, rfa.state_a[f], rfa.state_a[1 - f], rfa.state_c[f], rfa.state_c[1 - f], n,
                  torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
        rfa._flip = 1 - f

    # the torch memories' state in buffers that outlive every capture: Memory.forward leaves its state in a new tensor per step, and a graph
    # that read the warm-up's tensor would read freed memory once the allocator has released it (the next capture empties the cache)
    with torch.inference_mode():
        held = {m: tuple(torch.zeros(1, n, hidden, device=DEV) for _ in range(1 if gru else 2)) for m in (ac.memory_a, ac.memory_c)}

    def torch_stage():
        with torch.inference_mode():
            for m, buf in held.items():
                m.hidden_states = buf[0] if gru else buf
            ac.act(obs)
            ac.evaluate(obs)
            ac.reset(reset)
            for m, buf in held.items():                       # (four small copies the generic loop does not make)
                for dst, src in zip(buf, (m.hidden_states,) if gru else m.hidden_states):
                    dst.copy_(src)

    variants = {"device": (capture(device, args.graph_steps), device), "torch": (capture(torch_stage, args.graph_steps), torch_stage),
                "cell": (capture(cell, args.graph_steps), cell)}
    if gru:
        torch.manual_seed(1)
        lstm_ac = ActorCriticRecurrent(48, 48, 12, actor_hidden_dims=[128, 64, 32], critic_hidden_dims=[128, 64, 32], rnn_hidden_size=hidden).to(DEV)
        lstm_rfa = RecurrentFusedActor(lstm_ac, DEV, seed=3, num_envs=n)
        lstm = lambda: lstm_rfa.act_with_mean(obs, obs, reset=reset)
        variants["lstm"] = (capture(lstm, args.graph_steps), lstm)
    r = alternate(variants, args.graph_steps, args.replays, args.pairs, args.discard)
    flop = 2 * 2.0 * n * (48 + hidden) * (3 if gru else 4) * hidden
    r["cell"]["flop"] = flop
    r["cell"]["share_of_f32_mfma_peak"] = flop / (r["cell"]["median_us"] * 1e-6) / PEAK_F32_MFMA
    return r


def wide_against_narrow_cell(n, hidden, args):
    """``lg_lstm_wide_step`` against ``lg_lstm_step`` on the same two memories at a width both take."""
    from legged_games_gym_amd.rl import ActorCriticRecurrent
    from legged_games_gym_amd.rl.recurrent_actor import DeviceLstm, lstm_step
    torch.manual_seed(1)
    ac = ActorCriticRecurrent(48, 48, 12, actor_hidden_dims=[128, 64, 32], critic_hidden_dims=[128, 64, 32], rnn_hidden_size=hidden).to(DEV)
    obs = torch.rand(n, 48, device=DEV) * 6.0 - 3.0
    reset = (torch.rand(n, device=DEV) < 0.02).to(torch.uint8)
    variants = {}
    for name, wide in (("lg_lstm_wide_step", True), ("lg_lstm_step", False)):
        la, lc = DeviceLstm(ac.memory_a.rnn, DEV, wide=wide), DeviceLstm(ac.memory_c.rnn, DEV, wide=wide)
        st = [[(torch.zeros(n, hidden, device=DEV), torch.zeros(n, hidden, device=DEV)) for _ in range(2)] for _ in range(2)]
        flip = [0]

        def cell(la=la, lc=lc, st=st, flip=flip):
            f = flip[0]
            lstm_step(la.lib, la, lc, obs, obs, reset, st[0][f], st[0][1 - f], st[1][f], st[1][1 - f], n, torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
            flip[0] = 1 - f
        variants[name] = (capture(cell, args.graph_steps), cell)
    return alternate(variants, args.graph_steps, args.replays, args.pairs, args.discard)


def cell_only(n, hidden, launches):
    """``lg_lstm_step`` alone, eagerly, for a kernel trace."""
    from legged_games_gym_amd.rl import ActorCriticRecurrent
    from legged_games_gym_amd.rl.recurrent_actor import RecurrentFusedActor
    torch.manual_seed(1)
    ac = ActorCriticRecurrent(48, 48, 12, actor_hidden_dims=[128, 64, 32], critic_hidden_dims=[128, 64, 32], rnn_hidden_size=hidden).to(DEV)
    rfa = RecurrentFusedActor(ac, DEV, seed=3, num_envs=n)
    obs = torch.rand(n, 48, device=DEV) * 6.0 - 3.0
    for _ in range(launches):
        rfa.step_memories(obs, obs)
    torch.cuda.synchronize()
    print(json.dumps({"launches": launches, "num_envs": n, "hidden": hidden, "flop_per_launch": 2 * 2.0 * n * (48 + hidden) * 4 * hidden}))


def train_throughput(fused, iterations):
    from legged_games_gym_amd.envs import task_registry
    from legged_games_gym_amd.utils import get_args
    from legged_games_gym_amd.utils.helpers import apply_policy_args
    args = get_args(["--task", "anymal_c_flat", "--headless", "--sim_device", DEV, "--rl_device", DEV, "--policy_class_name", "ActorCriticRecurrent"])
    _, train_cfg = task_registry.get_cfgs("anymal_c_flat")
    apply_policy_args(train_cfg, args)
    train_cfg.runner.fused_rollout = fused
    env, _ = task_registry.make_env("anymal_c_flat", args)
    runner, _ = task_registry.make_alg_runner(env, "anymal_c_flat", args, log_root=None)
    runner.learn(1)
    torch.cuda.synchronize()
    t0 = time.time()
    runner.learn(iterations)
    torch.cuda.synchronize()
    dt = time.time() - t0
    return {"num_envs": env.num_envs, "steps_per_env": runner.num_steps_per_env, "iterations": iterations, "device_rollout": runner._fused is not None,
            "env_steps_per_s": iterations * env.num_envs * runner.num_steps_per_env / dt, "s_per_iteration": dt / iterations}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph-steps", type=int, default=50)
    ap.add_argument("--replays", type=int, default=4)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--discard", type=int, default=2)
    ap.add_argument("--envs", type=int, nargs="*", default=[2000, 4096])
    ap.add_argument("--hidden", type=int, nargs="*", default=[64, 256])
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--cell-only", action="store_true", help="launch the cell 200 times and exit (for a rocprofv3 kernel trace)")
    ap.add_argument("--train-iterations", type=int, default=3)
    ap.add_argument("--wide", action="store_true", help="measure liblegged_lstm_wide.so: 512 units, and the wide cell against lg_lstm_step at 256")
    ap.add_argument("--gru", action="store_true", help="measure liblegged_gru.so: GRU memories against torch and against the LSTM policy's device stage")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(REPO, "profiles", "recurrent_wide_step.json" if args.wide else "recurrent_gru_step.json" if args.gru else "recurrent_step.json")
    if args.wide:
        args.hidden, args.train = [512], False
    if args.gru:
        args.train = False
    if args.cell_only:
        return cell_only(4096, 256, 200)
    prime = torch.cuda.CUDAGraph()                      # the generator's graph-safe state, created outside inference_mode (rl/ppo.py)
    with torch.cuda.graph(prime, capture_error_mode="thread_local"):
        torch.zeros(1, device=DEV).add_(1.0)
    out = {"device_name": torch.cuda.get_device_name(0), "graph_steps": args.graph_steps, "replays": args.replays, "pairs": args.pairs, "stage": {}}
    for n in args.envs:
        for h in args.hidden:
            r = measure(n, h, args, wide=args.wide, gru=args.gru)
            out["stage"][f"{n}x{h}"] = r
            print(f"{n} envs, {h} units: " + "; ".join(f"{k} {v['median_us']:.1f} us [{v['min_us']:.1f} .. {v['max_us']:.1f}]" for k, v in r.items())
                  + f"; cell at {100 * r['cell']['share_of_f32_mfma_peak']:.1f} % of the f32-MFMA peak", flush=True)
    if args.wide:
        out["cell_at_256_units"] = {}
        for n in args.envs:
            out["cell_at_256_units"][f"{n}x256"] = r = wide_against_narrow_cell(n, 256, args)
            print(f"{n} envs, 256 units: " + "; ".join(f"{k} {v['median_us']:.1f} us [{v['min_us']:.1f} .. {v['max_us']:.1f}]" for k, v in r.items()), flush=True)
    if args.train:
        out["train"] = {}
        for fused in (True, False):
            out["train"]["fused_rollout" if fused else "generic_loop"] = r = train_throughput(fused, args.train_iterations)
            print(f"train, fused_rollout {fused}: {r['env_steps_per_s']:.0f} env steps/s ({r['s_per_iteration']:.3f} s per iteration)", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: {v: round(x["median_us"], 2) for v, x in r.items()} for k, r in out["stage"].items()}))


if __name__ == "__main__":
    main()
