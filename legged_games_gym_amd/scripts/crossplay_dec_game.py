"""Checkpoint cross-play of the decentralised predator-prey game: the predator of one checkpoint against the prey of another -- how progress
in alternating self-play is judged.

``python -m legged_games_gym_amd.scripts.crossplay_dec_game --task=dec_high_level_game --headless --load_run RUN --checkpoints 0,200,400
[--num_envs N --steps S]``

One env, one pair of ``FusedActor`` s and ONE captured deterministic policy-step graph (``scripts.play_dec_game.DecEvaluation``).  For every
pair (predator of checkpoint i, prey of checkpoint j) the two ``model_state_dict`` halves are loaded, ``sync_device()`` repacks them in
place underneath the graph, the env is put back to the same start -- the state a seeded ``env.reset()`` left, low-level step counter
included -- the outcome totals are zeroed, ``S`` steps (default: 2 x ``max_episode_length``) are replayed and the totals are read.  K x K
cells of ``S`` replays of a ~100 us step take seconds, so the envs of a launch are not grouped.

``crossplay_<i0>_..._<ik>.json`` in the run directory holds the K x K tables ``capture_rate``, ``timed_out_rate`` (the predator failed in
time) and ``mean_steps`` -- rows are predators, columns are preys -- and the raw totals of every cell.  As with ``play_dec_game --outcomes``,
episodes still running after ``S`` steps are not counted.  Recurrent checkpoints (``--policy_class_name ActorCriticRecurrent`` and the
``--rnn_*`` flags of the run): both ``RecurrentFusedActor`` s are repacked in place per cell, and every cell starts with all memories at zero
from the same start state as a feed-forward cell.  ``--privileged_critic {prey,pred,both}``: the flag of the run, so that the critics the
checkpoints are loaded into have their shape (``scripts.play_dec_game``)."""
import json
import os

import torch

from .play_dec_game import COUNTS, DecEvaluation, result_of
from .train_dec_game import _args as _train_args

TABLES = (("capture_rate", "captured_rate"), ("timed_out_rate", "timed_out_rate"), ("mean_steps", "mean_steps"))


def format_tables(checkpoints, tables):
    lines = []
    for name, _ in TABLES:
        lines.append(f"{name}: rows = predator of checkpoint, columns = prey of checkpoint")
        lines.append(f"{'':>10}" + "".join(f"{c:>10}" for c in checkpoints))
        for i, row in zip(checkpoints, tables[name]):
            lines.append(f"{i:>10}" + "".join(f"{'-':>10}" if v is None else f"{v:>10.3f}" for v in row))
    lines.append("episodes still running at the end of a cell are not counted, which favours short episodes")
    return "\n".join(lines)


def crossplay(args, checkpoints, steps=None):
    """-> (DecEvaluation, result dict as written to the JSON file, path of the file)."""
    checkpoints = [int(c) for c in checkpoints]
    if not checkpoints:
        raise SystemExit("--checkpoints needs at least one iteration, e.g. --checkpoints 0,200,400")
    args.checkpoint = checkpoints[0]             # the env, the actors and the graph are built on the first checkpoint
    ev = DecEvaluation(args)
    run_dir = os.path.dirname(ev.checkpoint)
    halves = {}
    for c in dict.fromkeys(checkpoints):
        d = torch.load(os.path.join(run_dir, f"model_{c}.pt"), map_location=ev.env.device, weights_only=True)
        halves[c] = {a: d[a]["model_state_dict"] for a in ("pred", "prey")}
    n = int(steps) if steps is not None else 2 * int(ev.env.max_episode_length)
    tables = {name: [] for name, _ in TABLES}
    totals = []
    for i in checkpoints:                        # rows: predators
        row_totals = []
        for name, _ in TABLES:
            tables[name].append([])
        for j in checkpoints:                    # columns: preys
            ev.load(halves[i]["pred"], halves[j]["prey"])
            cell = ev.run(n)
            _, pieces = result_of(cell)
            flat = dict(pieces["rates"], mean_steps=pieces["mean_steps"])
            for name, key in TABLES:
                tables[name][-1].append(flat[key])
            row_totals.append({k: int(cell[k]) for k in COUNTS})
        totals.append(row_totals)
    result = dict(task=args.task, checkpoints=checkpoints, num_envs=int(ev.env.num_envs), steps=n, path=ev.path, rows="predator", columns="prey",
                  totals=totals, **tables)
    print(f"{ev.env.num_envs} envs x {n} high-level steps per cell, {ev.path}")
    print(format_tables(checkpoints, tables))
    out = os.path.join(run_dir, "crossplay_" + "_".join(str(c) for c in checkpoints) + ".json")
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print("written to:", out)
    return ev, result, out


def _args(argv=None):
    import argparse
    import sys
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument("--steps", type=int, default=None, help="high-level steps per cell (default: 2 x max_episode_length)")
    pre.add_argument("--checkpoints", type=str, required=True, help="comma-separated iterations of one run, e.g. 0,200,400")
    own, rest = pre.parse_known_args(list(sys.argv[1:] if argv is None else argv))
    args = _train_args(rest)
    args.steps, args.checkpoints = own.steps, [int(c) for c in own.checkpoints.split(",") if c.strip()]
    return args


if __name__ == "__main__":
    _a = _args()
    crossplay(_a, _a.checkpoints, steps=_a.steps)
