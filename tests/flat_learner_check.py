"""Shared pieces of tests/test_gpu_flat_learner.py (GPU) and tests/test_flat_learner_check.py (CPU): the host rule of the LDS-resident
learner kernels (csrc/lg_learner.hip: mlp_fill) restated, and the mini-batch sizes and layer widths derived from it at which
k_mlp_train / k_mlp_reduce (csrc/lg_train.h) change path.  Nothing here touches the device library, so the derivation is tested
without a GPU."""
from collections import namedtuple

HIDDEN = (128, 64, 32)                    # mlp_fill refuses every other hidden shape
TILE = 16                                 # rows of one row tile
TRAIN_WGS = 256                           # LG_TRAIN_WGS: partial-sum slices of the backward builds
BUILDS = {"forward": (4, False), "backward": (2, True)}       # build -> (LG_FWD_SLOTS | LG_BWD_SLOTS, writes partials); the fused build is "backward"

# actor input widths: scalar path of LdsFill::load / request() (1, 3, 17, 47), mixed path (% 4 == 0, not % 16: 4, 44), a wave with
# no live input column (1, 3, 4: waves 1 and 2; 17, 32: wave 2), the full vector path (32, 48)
ACTOR_INPUTS = (1, 3, 4, 17, 32, 44, 47, 48)
# output widths: lane groups of a row wholly idle (< 4 per missing group), quad() loads scalar (d4 & 3), 16: none idle
OUTPUTS = (1, 2, 3, 4, 5, 12, 13, 16)
CRITIC_PAIRS = ((48, 17), (3, 44), (47, 47))                  # (actor inputs, critic inputs): two nets with separate input tables
REDUCE_PARTIALS = (2, 7, 8, 9, 15, 16, 17, 25)                # k_mlp_reduce: for (; k + 8 < n; k += 16) and its tail, on every side of 8 / 16 / 24

Case = namedtuple("Case", "id build n_nets mb n_tiles wgs n_iter idle")     # wgs .. idle: what the derivation below says mlp_fill will do


def schedule(mb, n_nets, slots, partials, cus):
    """mlp_fill restated: (row tiles, workgroups per net = partials summed by k_mlp_reduce, trips of the persistent loop,
    4-wave groups with no row tile in the last trip)."""
    n_tiles = (mb + TILE - 1) // TILE
    wgs = cus // n_nets
    if partials:
        wgs = min(wgs, TRAIN_WGS)
    if wgs * slots > n_tiles:
        wgs = (n_tiles + slots - 1) // slots
    wgs = max(wgs, 1)
    n_iter = (n_tiles + wgs * slots - 1) // (wgs * slots)
    return n_tiles, wgs, n_iter, wgs * slots * n_iter - n_tiles


def mb_cases(cus):
    """Mini-batch sizes of the schedule tests for a part with ``cus`` compute units; the ids do not depend on ``cus``."""
    out = []

    def add(cid, build, n_nets, n_tiles, short, wgs, n_iter):
        slots = BUILDS[build][0]
        out.append(Case(f"{build}{n_nets}-{cid}", build, n_nets, TILE * n_tiles - short, n_tiles, wgs, n_iter, wgs * slots * n_iter - n_tiles))

    for n_nets in (2, 1):
        c_bwd, c_fwd = min(cus // n_nets, TRAIN_WGS), cus // n_nets
        assert c_bwd >= max(REDUCE_PARTIALS), "too few compute units for the largest partial count"
        # backward and fused build: one tile (1, 15, 16 rows), two tiles with one row in the second
        for mb in (1, 15, 16, 17) if n_nets == 2 else (1, 17):
            n_tiles = (mb + TILE - 1) // TILE
            add(f"mb{mb}", "backward", n_nets, n_tiles, TILE * n_tiles - mb, 1, 1)
        if n_nets == 2:
            for k in REDUCE_PARTIALS:                                           # k partials, an idle slot in the last workgroup, a ragged last tile
                add(f"partials{k}", "backward", n_nets, 2 * k - 1, 3, k, 1)
        add("trip2", "backward", n_nets, 2 * c_bwd + 1, 5, c_bwd, 2)             # second trip: one live group
        if n_nets == 2:
            add("trip3", "backward", n_nets, 4 * c_bwd + 3, 5, c_bwd, 3)         # third trip: request() / row_index() one and two tiles ahead
        for mb in (1, 17, 49, 65) if n_nets == 2 else (1, 65):
            n_tiles = (mb + TILE - 1) // TILE
            add(f"mb{mb}", "forward", n_nets, n_tiles, TILE * n_tiles - mb, (n_tiles + 3) // 4, 1)
        add("trip2", "forward", n_nets, 4 * c_fwd + 1, 5, c_fwd, 2)
        if n_nets == 2:
            add("trip3", "forward", n_nets, 8 * c_fwd + 2, 5, c_fwd, 3)
    return out


CASE_IDS = {build: [c.id for c in mb_cases(TRAIN_WGS) if c.build == build] for build in BUILDS}


def case(cus, cid):
    return next(c for c in mb_cases(cus) if c.id == cid)


def rows_with_duplicates(gen, mb, table_rows):
    """``mb`` row indices (int64, CPU) of a table of ``table_rows`` rows: a third of them copies of others, with the first and the
    last table row among them, in random order."""
    import torch
    n_dup = mb // 3
    distinct = torch.randperm(table_rows - 2, generator=gen)[:mb - n_dup - 2] + 1
    distinct = torch.cat((torch.tensor([0, table_rows - 1]), distinct))
    dup = distinct[torch.randint(distinct.numel(), (n_dup,), generator=gen)]
    rows = torch.cat((distinct, dup))
    return rows[torch.randperm(mb, generator=gen)]
