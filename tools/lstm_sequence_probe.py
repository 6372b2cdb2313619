"""The recurrence of a recurrent policy's PPO update on the device kernels against ``nn.LSTM`` + autograd -> profiles/lstm_sequence.json.

One process, HIP events, the variants alternated over repeats, median [min .. max] per variant; eager launches (the recurrent update is not
captured in a graph), ``--inner`` calls between two events.  Every tensor a variant touches lives as long as the process.

(a) one memory, forward + backward over T = 24 steps of B = 1024 and 2048 trajectories, (inputs, units) = (48, 64), (48, 256), (235, 256):

  device    DeviceLstmSequence: pack + lg_lstm_seq_forward, then lg_lstm_seq_backward + the three dW / db GEMMs in torch
  torch     nn.LSTM forward and autograd backward on the same tensors
  kernels   the pack, forward and backward launches alone (no dW GEMMs): the serial part by itself

(b) ``PPO.update`` of anymal_c_flat at 4096 envs with a 256-unit ActorCriticRecurrent, ``device_bptt`` on and off: ONE runner and ONE stored
rollout, the two memories' ``sequence`` attached and detached between repeats, so both variants see the same storage.

Run on the GPU: ``python tools/lstm_sequence_probe.py [--no-update]``."""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
sys.path.insert(0, REPO)
DEV = "cuda:0"
T = 24


def alternate(variants, inner, pairs, discard):
    times = {k: [] for k in variants}
    for pair in range(pairs + discard):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            torch.cuda.synchronize()
            if pair >= discard:
                times[name].append(a.elapsed_time(b) * 1000.0 / inner)
    return {k: {"median_us": sorted(v)[len(v) // 2], "min_us": min(v), "max_us": max(v), "repeats_us": v} for k, v in times.items()}


def one_memory(B, I, H, args):
    from legged_games_gym_amd.rl.lstm_sequence import DeviceLstmSequence
    torch.manual_seed(1)
    rnn = nn.LSTM(I, H).to(DEV)
    seq = DeviceLstmSequence(rnn, DEV)
    lengths = torch.randint(1, T + 1, (B,), device=DEV)
    live = (torch.arange(T, device=DEV).unsqueeze(1) < lengths.unsqueeze(0)).float().unsqueeze(-1)
    x = (torch.rand(T, B, I, device=DEV) * 6.0 - 3.0) * live
    dh = torch.randn(T, B, H, device=DEV) * live
    state = (torch.rand(1, B, H, device=DEV) - 0.5, torch.rand(1, B, H, device=DEV) - 0.5)
    h_out, ws = torch.empty(T, B, H, device=DEV), torch.empty(5 * T * B * H, device=DEV)
    stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    ps = [p.data_ptr() for p in (rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0)]

    def device():
        rnn.zero_grad(set_to_none=True)
        seq(x, state).backward(dh)

    def torch_lstm():
        rnn.zero_grad(set_to_none=True)
        rnn(x, state)[0].backward(dh)

    def kernels():
        lib = seq.lib
        rc = lib.lg_lstm_seq_load_device(seq.handle, *ps, stream)
        rc = rc or lib.lg_lstm_seq_forward(seq.handle, x.data_ptr(), x.stride(0), state[0].data_ptr(), state[1].data_ptr(), h_out.data_ptr(), ws.data_ptr(), T, B, stream)
        rc = rc or lib.lg_lstm_seq_backward(seq.handle, ps[1], dh.data_ptr(), state[1].data_ptr(), ws.data_ptr(), T, B, stream)
        if rc:
            raise RuntimeError(lib.lg_lstm_seq_last_error().decode())

    for fn in (device, torch_lstm, kernels):                 # warm-up: allocator, MIOpen's choice of algorithm
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    return alternate({"device": device, "torch": torch_lstm, "kernels": kernels}, args.inner, args.pairs, args.discard)


def ppo_update(args):
    from legged_games_gym_amd.envs import task_registry
    from legged_games_gym_amd.utils import get_args
    from legged_games_gym_amd.utils.helpers import apply_policy_args
    cli = get_args(["--task", "anymal_c_flat", "--headless", "--num_envs", "4096", "--sim_device", DEV, "--rl_device", DEV,
                    "--policy_class_name", "ActorCriticRecurrent", "--rnn_hidden_size", "256"])
    _, train_cfg = task_registry.get_cfgs("anymal_c_flat")
    apply_policy_args(train_cfg, cli)
    train_cfg.runner.device_bptt = True
    env, _ = task_registry.make_env("anymal_c_flat", cli)
    runner, _ = task_registry.make_alg_runner(env, "anymal_c_flat", cli, log_root=None)
    alg, ac = runner.alg, runner.alg.actor_critic
    attached = ac.memory_a.sequence, ac.memory_c.sequence
    assert attached[0] is not None and attached[1] is not None
    runner.learn(1)                                           # one rollout: the storage every update below reads (update() leaves it in place)
    torch.cuda.synchronize()

    def on():
        ac.memory_a.sequence, ac.memory_c.sequence = attached
        alg.update()

    def off():
        ac.memory_a.sequence = ac.memory_c.sequence = None
        alg.update()

    for fn in (on, off):
        fn()
    torch.cuda.synchronize()
    r = alternate({"device_bptt_on": on, "device_bptt_off": off}, 1, args.pairs, args.discard)
    n_traj = int(next(iter(alg.storage.recurrent_mini_batch_generator(alg.num_mini_batches, 1)))[0].shape[1])
    r["shape"] = {"num_envs": env.num_envs, "steps_per_env": runner.num_steps_per_env, "mini_batches": alg.num_mini_batches, "epochs": alg.num_learning_epochs,
                  "trajectories_in_first_mini_batch": n_traj, "units": 256}
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--discard", type=int, default=2)
    ap.add_argument("--no-update", action="store_true", help="skip (b), the PPO update of anymal_c_flat")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lstm_sequence.json"))
    args = ap.parse_args()
    out = {"device_name": torch.cuda.get_device_name(0), "T": T, "inner": args.inner, "pairs": args.pairs, "one_memory": {}}
    for B in (1024, 2048):
        for I, H in ((48, 64), (48, 256), (235, 256)):
            out["one_memory"][f"B{B}_I{I}_H{H}"] = r = one_memory(B, I, H, args)
            print(f"B {B}, {I} inputs, {H} units: " + "; ".join(f"{k} {v['median_us']:.0f} us [{v['min_us']:.0f} .. {v['max_us']:.0f}]" for k, v in r.items()), flush=True)
    if not args.no_update:
        out["ppo_update"] = r = ppo_update(args)
        print("PPO.update, anymal_c_flat, 4096 envs, 256 units: " + "; ".join(
            f"{k} {r[k]['median_us'] / 1000:.1f} ms [{r[k]['min_us'] / 1000:.1f} .. {r[k]['max_us'] / 1000:.1f}]" for k in ("device_bptt_on", "device_bptt_off")), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
