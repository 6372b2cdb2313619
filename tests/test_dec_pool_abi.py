"""The decentralised game's opponent pool without a GPU: the header's functions are ``capi.DEC_POOL_SYMBOLS`` (include/legged_dec_game_pool.h),
the built library exports them with the ctypes layout and refuses bad arguments before any launch or allocation, the row of the kernel
resource table, the block assignment ``rl.opponent_pool.assign_blocks`` and the command-line flags of ``train_dec_game``."""
import ctypes
import os
import re

import pytest
import torch

from legged_games_gym_amd import capi

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
RESOURCES = os.path.join(REPO, "legged_games_gym_amd", "csrc", "kernel_resources.txt")
HEADER = "legged_dec_game_pool.h"
OTHER = {"legged_hip.h": "EXPORTED_SYMBOLS", "legged_game.h": "GAME_SYMBOLS", "legged_dec_game.h": "DEC_GAME_SYMBOLS", "legged_pursuer_game.h": "PURSUER_SYMBOLS",
         "legged_game_outcome.h": "OUTCOME_SYMBOLS", "legged_dec_game_outcome.h": "DEC_OUTCOME_SYMBOLS"}
FORBIDDEN = ("k_dec_", "k_game_", "k_prey_act", "k_policy_act", "k_pursuer_post", "k_outcome_post", "k_step", "k_physics")      # substrings existing tests count rows by


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", header)).read(), flags=re.S)
    return re.findall(r"\b(lg_[a-z_0-9]+)\s*\(", text)


@pytest.fixture(scope="module")
def lib():
    path = capi.library_path()
    if not os.path.isfile(path):
        import __graft_entry__ as entry
        entry.build()
    lib = ctypes.CDLL(path)
    lib.lg_last_error.restype = ctypes.c_char_p
    return lib


def test_header_symbol_list_matches_binding_and_is_disjoint_from_the_others():
    assert sorted(_declared(HEADER)) == sorted(capi.DEC_POOL_SYMBOLS)
    assert {"lg_dec_pool_create", "lg_dec_pool_destroy", "lg_dec_pool_act", "lg_dec_pool_sizeof"} <= set(capi.DEC_POOL_SYMBOLS)
    for header, name in OTHER.items():
        assert not set(capi.DEC_POOL_SYMBOLS) & set(getattr(capi, name)), name
        assert not set(capi.DEC_POOL_SYMBOLS) & set(_declared(header)), header
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", HEADER)).read(), flags=re.S)
    assert "LG_ABI_VERSION" not in text and capi.LG_ABI_VERSION == 22
    assert re.search(r"#define\s+LG_DEC_POOL_MAX\s+16\b", text) and capi.LG_DEC_POOL_MAX == 16
    assert re.search(r"#define\s+LG_DEC_POOL_BLOCK_ENVS\s+32\b", text) and capi.LG_DEC_POOL_BLOCK_ENVS == 32
    assert "stream capture" in open(os.path.join(REPO, "include", HEADER)).read()          # pool creation is not allowed inside one: the header says so
    # the 20-argument plain entry point is untouched
    capi_args = 20
    plain = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "legged_dec_game.h")).read(), flags=re.S)
    assert re.search(r"int lg_dec_game_act\(([^;]*)\);", plain).group(1).count(",") == capi_args - 1


def test_library_exports_the_symbols_with_the_ctypes_layout(lib):
    for sym in capi.DEC_POOL_SYMBOLS:
        assert hasattr(lib, sym), sym
    lib.lg_dec_pool_sizeof.argtypes, lib.lg_dec_pool_sizeof.restype = [ctypes.c_int], ctypes.c_int
    assert lib.lg_dec_pool_sizeof(0) == ctypes.sizeof(capi.lg_dec_pool_info) == 4 * 4 + ctypes.sizeof(ctypes.c_void_p)
    assert lib.lg_dec_pool_sizeof(1) == -1 and lib.lg_dec_pool_sizeof(-1) == -1
    capi.bind_header(lib, "legged_dec_game_pool.h")                                          # raises on a layout mismatch
    assert len(lib.lg_dec_pool_act.argtypes) == 24                              # the 20 of lg_dec_game_act and two (pool, slot table) pairs
    lib.lg_abi_version.restype = ctypes.c_int
    assert lib.lg_abi_version() == 22


def _act(lib, pred=0x1000, prey=0x1000, ll=0x1000, pool_pred=None, slot_pred=None, pool_prey=None, slot_prey=None, seeds=(1, 2), num_envs=8, buffers=None):
    """``lg_dec_pool_act`` on addresses that are never dereferenced: every call below is refused first."""
    P = capi.lg_dec_game_params()
    P.num_envs, P.decimation = num_envs, 4
    B = capi.dec_game_buffers({name: 0x1000 for name in capi.DEC_GAME_BUFFER_FIELDS} if buffers is None else buffers)
    return lib.lg_dec_pool_act(pred, prey, ll, pool_pred, slot_pred, pool_prey, slot_prey, ctypes.byref(P), ctypes.byref(B), 0x1000, 0x1000, 0x1000, 0x1000, 0x1000,
                               0x1000, seeds[0], seeds[1], 1, None, 0, 0, None, None, None)


def test_bad_arguments_are_refused_before_any_launch_or_allocation(lib):
    capi.bind_header(lib, "legged_dec_game_pool.h")
    out = ctypes.c_void_p()
    members = (ctypes.c_void_p * 17)(*([0x1000] * 17))                          # never dereferenced: count and role are checked first
    assert lib.lg_dec_pool_create(None, 1, 1, 0, ctypes.byref(out)) == -1
    assert lib.lg_dec_pool_create(members, 1, 1, 0, None) == -1
    for count in (0, 17, -3):
        assert lib.lg_dec_pool_create(members, count, 1, 0, ctypes.byref(out)) == -2 and b"count" in lib.lg_last_error(), count
    for role in (0, 3):
        assert lib.lg_dec_pool_create(members, 2, role, 0, ctypes.byref(out)) == -2 and b"role" in lib.lg_last_error(), role
    nulls = (ctypes.c_void_p * 2)(None, None)
    assert lib.lg_dec_pool_create(nulls, 2, 1, 0, ctypes.byref(out)) == -1 and b"member" in lib.lg_last_error()
    assert not out.value
    assert lib.lg_dec_pool_destroy(None) == -1 and lib.lg_dec_pool_query(None, None) == -1
    # the act entry point: a pool given without its slot table, for either role
    assert _act(lib, pool_prey=0x1000, slot_prey=None) == -1 and b"block_slot" in lib.lg_last_error()
    assert _act(lib, pool_pred=0x1000, slot_pred=None) == -1 and b"block_slot" in lib.lg_last_error()
    # a role with neither handle nor pool; a null params struct; a missing command buffer
    assert _act(lib, prey=None) == -1 and _act(lib, pred=None) == -1 and _act(lib, ll=None) == -1
    assert lib.lg_dec_pool_act(0x1000, 0x1000, 0x1000, None, None, None, None, None, None, 0x1000, 0x1000, 0x1000, 0x1000, 0x1000, 0x1000, 1, 2, 1, None, 0, 0,
                               None, None, None) == -1
    assert _act(lib, buffers={k: (0 if k == "ll_commands" else 0x1000) for k in capi.DEC_GAME_BUFFER_FIELDS}) == -1
    assert _act(lib, num_envs=0) == -2 and b"num_envs" in lib.lg_last_error()
    # equal seeds: the sampled roles share their noise purposes
    assert _act(lib, seeds=(5, 5)) == -2 and b"must differ" in lib.lg_last_error()


def test_kernel_resource_table_lists_the_pool_kernel_and_keeps_the_others():
    rows = [l for l in open(RESOURCES) if not l.startswith("#")]
    fields = lambda row: dict(zip(row.split()[1::2], map(int, row.split()[2::2])))
    mine = [l for l in rows if "k_pool_act" in l]
    assert len(mine) == 1, mine
    f = fields(mine[0])
    wide = [fields(l) for l in rows if "k_policy_act_wide" in l]
    assert wide and f["spill"] == 0 and f["scratch"] == 0 and 0 < f["LDS"] <= max(w["LDS"] for w in wide), mine[0]
    for sub in FORBIDDEN:
        assert sub not in mine[0].split()[0], (sub, mine[0])
    assert len([l for l in rows if "k_step" in l or "k_physics" in l]) == 32
    plain = [l for l in rows if "k_dec_act" in l]
    assert len(plain) == 1
    g = fields(plain[0])
    assert g["spill"] == 0 and g["scratch"] == 0 and g["LDS"] == f["LDS"] and f["occupancy"] == g["occupancy"], (plain[0], mine[0])


@pytest.mark.parametrize("blocks,filled,share", [(1, 0, 0.5), (4, 0, 0.5), (63, 3, 0.5), (63, 3, 0.0), (63, 3, 1.0), (128, 15, 0.25)])
def test_assign_blocks_counts(blocks, filled, share):
    from legged_games_gym_amd.rl.opponent_pool import assign_blocks
    slots = assign_blocks(blocks, filled, share, torch.Generator().manual_seed(7))
    assert slots.dtype == torch.int32 and slots.shape == (blocks,)
    counts = torch.bincount(slots.long(), minlength=filled + 1).tolist()
    assert len(counts) == filled + 1 and int(slots.min()) >= 0                    # only slots 0 .. filled appear
    live = blocks if filled == 0 else (0 if share == 0 else min(blocks, max(1, round(share * blocks))))
    assert counts[0] == live, counts
    if filled:
        assert sum(counts[1:]) == blocks - live and max(counts[1:]) - min(counts[1:]) <= 1, counts
    want = {(1, 0, 0.5): [1], (4, 0, 0.5): [4], (63, 3, 0.5): [32, 11, 10, 10], (63, 3, 0.0): [0, 21, 21, 21], (63, 3, 1.0): [63, 0, 0, 0]}.get((blocks, filled, share))
    if want is not None:
        assert sorted(counts[1:], reverse=True) == want[1:] and counts[0] == want[0], counts
    else:
        assert counts[0] == 32 and sorted(counts[1:], reverse=True) == [7] * 6 + [6] * 9, counts      # 96 blocks over 15 snapshots
    assert torch.equal(slots, assign_blocks(blocks, filled, share, torch.Generator().manual_seed(7)))     # the same seed, the same table


def test_assign_blocks_depends_on_the_seed_and_scatters_the_live_blocks():
    from legged_games_gym_amd.rl.opponent_pool import assign_blocks
    a = assign_blocks(63, 3, 0.5, torch.Generator().manual_seed(7))
    b = assign_blocks(63, 3, 0.5, torch.Generator().manual_seed(8))
    assert not torch.equal(a, b) and torch.bincount(a.long()).tolist() == torch.bincount(b.long()).tolist()
    live = (a == 0).nonzero().flatten().tolist()
    assert live != list(range(live[0], live[0] + len(live)))                     # by block at random, not one contiguous env range
    with pytest.raises(ValueError):
        assign_blocks(0, 0, 0.5, None)
    with pytest.raises(ValueError):
        assign_blocks(4, 1, 1.5, None)


def test_the_pool_is_two_flags_and_two_runner_keys_but_no_config_field():
    from legged_games_gym_amd.envs.a1_game import DecHighLevelGameCfgPPO
    from legged_games_gym_amd.scripts import train_dec_game
    from legged_games_gym_amd.utils.helpers import class_to_dict
    args = train_dec_game._args(["--opponent_pool", "4", "--opponent_latest_share", "0.25"])
    assert args.opponent_pool == 4 and args.opponent_latest_share == 0.25
    d = train_dec_game._args([])
    assert d.opponent_pool == 0 and d.opponent_latest_share == 0.5
    runner = class_to_dict(DecHighLevelGameCfgPPO())["runner"]
    assert "opponent_pool_size" not in runner and "opponent_latest_share" not in runner
