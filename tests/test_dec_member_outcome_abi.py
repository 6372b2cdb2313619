"""The outcome statistics per pool member without a GPU: the header's functions are ``capi.DEC_MEMBER_OUTCOME_SYMBOLS`` (include/
legged_dec_game_member_outcome.h), the built library exports them with the ctypes layout and refuses bad arguments before any launch, the row
of the kernel resource table, the NumPy twin and the seeded cases the device tests use, the pure functions of the prioritised deal
(``rl/opponent_pool.py``), and the runner's refusal of ``opponent_priority`` without what it needs."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from legged_games_gym_amd import capi

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
RESOURCES = os.path.join(REPO, "legged_games_gym_amd", "csrc", "kernel_resources.txt")
HEADER = "legged_dec_game_member_outcome.h"
OTHER = {"legged_hip.h": "EXPORTED_SYMBOLS", "legged_game.h": "GAME_SYMBOLS", "legged_dec_game.h": "DEC_GAME_SYMBOLS", "legged_pursuer_game.h": "PURSUER_SYMBOLS",
         "legged_game_outcome.h": "OUTCOME_SYMBOLS", "legged_dec_game_outcome.h": "DEC_OUTCOME_SYMBOLS", "legged_dec_game_pool.h": "DEC_POOL_SYMBOLS"}
FORBIDDEN = ("k_dec_", "k_pool_act", "k_outcome_post", "k_game_", "k_prey_act", "k_policy_act", "k_pursuer_post", "k_step", "k_physics")      # substrings existing tests count rows by


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
    assert sorted(_declared(HEADER)) == sorted(capi.DEC_MEMBER_OUTCOME_SYMBOLS) == sorted(["lg_dec_member_outcome_post", "lg_dec_member_outcome_sizeof"])
    for header, name in OTHER.items():
        assert not set(capi.DEC_MEMBER_OUTCOME_SYMBOLS) & set(getattr(capi, name)), name
        assert not set(capi.DEC_MEMBER_OUTCOME_SYMBOLS) & set(_declared(header)), header
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", HEADER)).read(), flags=re.S)
    assert "LG_ABI_VERSION" not in text and capi.LG_ABI_VERSION == 22
    assert re.search(r"#define\s+LG_DEC_MEMBER_OUTCOME_ROWS\s+LG_DEC_POOL_MAX\b", text) and capi.LG_DEC_MEMBER_OUTCOME_ROWS == capi.LG_DEC_POOL_MAX == 16
    import __graft_entry__ as entry
    assert "lg_member_outcome.hip" in entry.HIP_SOURCES and "lg_member_outcome_entry.h" in entry.HIP_HEADERS
    assert any(h.endswith(os.path.join("include", HEADER)) for h in entry.HIP_HEADERS)


def test_library_exports_the_symbols_with_the_ctypes_layout(lib):
    for sym in capi.DEC_MEMBER_OUTCOME_SYMBOLS:
        assert hasattr(lib, sym), sym
    lib.lg_dec_member_outcome_sizeof.argtypes, lib.lg_dec_member_outcome_sizeof.restype = [ctypes.c_int], ctypes.c_int
    assert lib.lg_dec_member_outcome_sizeof(0) == ctypes.sizeof(capi.lg_dec_member_outcome_buffers) == 3 * ctypes.sizeof(ctypes.c_void_p) + 2 * 4
    assert lib.lg_dec_member_outcome_sizeof(1) == -1 and lib.lg_dec_member_outcome_sizeof(-1) == -1
    capi.bind_header(lib, "legged_dec_game_member_outcome.h")                                # raises on a layout mismatch
    assert [name for name, _ in capi.lg_dec_member_outcome_buffers._fields_] == ["block_slot", "member_accum", "member_totals", "count", "_pad"]
    lib.lg_abi_version.restype = ctypes.c_int
    assert lib.lg_abi_version() == 22


def _arguments(num_envs=8, count=3):
    """Parameters and pointer tables that pass every check (the addresses are never dereferenced: each call below is refused first)."""
    P = capi.lg_dec_game_params()
    P.num_envs, P.decimation, P.max_episode_length_s = num_envs, 4, 20.0
    B = capi.dec_game_buffers({name: 0x1000 for name in capi.DEC_GAME_BUFFER_FIELDS})
    O = capi.dec_outcome_buffers({name: 0x1000 for name in capi.DEC_OUTCOME_BUFFER_FIELDS})
    M = capi.dec_member_outcome_buffers({name: 0x1000 for name in capi.DEC_MEMBER_OUTCOME_BUFFER_FIELDS}, count)
    return P, B, O, M


def test_bad_arguments_are_refused_before_any_launch(lib):
    capi.bind_header(lib, "legged_dec_game_member_outcome.h")
    post, r = lib.lg_dec_member_outcome_post, ctypes.byref
    P, B, O, M = _arguments()
    # a null struct; the new one is named
    assert post(None, r(B), r(O), r(M), 3, None) == -1 and post(r(P), None, r(O), r(M), 3, None) == -1
    assert post(r(P), r(B), None, r(M), 3, None) == -1 and b"lg_dec_outcome_buffers" in lib.lg_last_error()
    assert post(r(P), r(B), r(O), None, 3, None) == -1 and b"lg_dec_member_outcome_buffers" in lib.lg_last_error()
    # a null buffer: the game's, the outcome's, the new struct's
    for name in ("ll_root_states", "obs_prey", "reset_buf", "episode_means", "extras_accum", "extras_ticket", "command_pred"):
        Bn = capi.dec_game_buffers({k: (0 if k == name else 0x1000) for k in capi.DEC_GAME_BUFFER_FIELDS})
        assert post(r(P), r(Bn), r(O), r(M), 3, None) == -1, name
    for name in capi.DEC_OUTCOME_BUFFER_FIELDS:
        On = capi.dec_outcome_buffers({k: (0 if k == name else 0x1000) for k in capi.DEC_OUTCOME_BUFFER_FIELDS})
        assert post(r(P), r(B), r(On), r(M), 3, None) == -1 and b"lg_dec_outcome_buffers" in lib.lg_last_error(), name
    for name in capi.DEC_MEMBER_OUTCOME_BUFFER_FIELDS:
        Mn = capi.dec_member_outcome_buffers({k: (0 if k == name else 0x1000) for k in capi.DEC_MEMBER_OUTCOME_BUFFER_FIELDS}, 3)
        assert post(r(P), r(B), r(O), r(Mn), 3, None) == -1 and b"lg_dec_member_outcome_buffers" in lib.lg_last_error(), name
    # count outside 1 .. 16
    for count in (0, -1, 17, 1 << 20):
        Mc = _arguments(count=count)[3]
        assert post(r(P), r(B), r(O), r(Mc), 3, None) == -2 and b"count" in lib.lg_last_error(), count
    # the errors of lg_dec_outcome_post carry over
    assert post(r(_arguments(num_envs=0)[0]), r(B), r(O), r(M), 3, None) == -2 and b"num_envs" in lib.lg_last_error()
    Pz = _arguments()[0]
    Pz.max_episode_length_s = 0.0
    assert post(r(Pz), r(B), r(O), r(M), 3, None) == -2 and b"max_episode_length_s" in lib.lg_last_error()
    Bs = capi.dec_game_buffers({k: (0 if k == "ll_step_counter" else 0x1000) for k in capi.DEC_GAME_BUFFER_FIELDS})
    assert post(r(P), r(Bs), r(O), r(M), -1, None) == -9
    # the wrapper raises with the code
    with pytest.raises(RuntimeError, match=r"\(-2\)"):
        capi.dec_member_outcome_post(P, B, O, _arguments(count=0)[3], 3)


def test_kernel_resource_table_lists_the_member_kernel_and_keeps_the_others():
    rows = [l for l in open(RESOURCES) if not l.startswith("#")]
    fields = lambda row: dict(zip(row.split()[1::2], map(int, row.split()[2::2])))
    mine = [l for l in rows if "k_member_outcome" in l]
    assert len(mine) == 1, mine
    f = fields(mine[0])
    assert f["spill"] == 0 and f["scratch"] == 0 and f["AGPRs"] == 0 and f["VGPRs"] <= 64 and 256 < f["LDS"] <= 2048, mine[0]
    assert f["occupancy"] >= 1                                                   # recorded, not required
    for sub in FORBIDDEN:
        assert sub not in mine[0].split()[0], (sub, mine[0])
    assert len([l for l in rows if "k_dec_outcome" in l]) == 1 and len([l for l in rows if "k_dec_post" in l]) == 1
    assert len([l for l in rows if "k_pool_act" in l]) == 1 and len([l for l in rows if "k_step" in l or "k_physics" in l]) == 32


def test_twin_groups_by_the_clamped_slot_of_the_block_and_the_seeded_cases_cannot_pass_empty():
    from tests import dec_member_outcome_fixtures as mf
    from tests import dec_member_outcome_twin as mt
    from tests import dec_outcome_twin as ot
    # a hand-made step of 70 envs (three blocks, the last with 6 envs): env 3 is captured, timed out and fallen at once
    n = 70
    z = lambda: np.zeros(n, bool)
    capture, time_out, ll_reset, ll_time_out = z(), z(), z(), z()
    capture[[3, 40]], time_out[[3, 65]], ll_reset[[3, 33, 69]], ll_time_out[[33]] = True, True, True, True
    f = ot.flags(dict(capture=capture, time_out=time_out, done=capture | time_out | ll_reset), ll_reset, ll_time_out)
    step = np.arange(n, dtype=np.int64)
    got = mt.member_counts(f, step, [2, -3, 99], 5)                              # block 0 -> 2, block 1 -> 0 (clamped), block 2 -> 4 (clamped)
    want = np.zeros((16, 6), np.int64)
    want[2], want[0], want[4] = [1, 1, 1, 1, 0, 4], [2, 1, 0, 0, 1, 34 + 41], [2, 0, 1, 1, 0, 66 + 70]
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(mt.member_counts(f, step, [2, -3, 99], 1)[0], ot.counts(f, step))      # count 1: everything is member 0's
    assert mt.env_member([5, 1], 33, 16).tolist() == [5] * 32 + [1]
    # the cases the device tests launch
    assert mf.SIZES == (1, 31, 32, 33, 64, 255, 256, 257, 300, 2000)
    for n in mf.SIZES:
        c = mf.case(n)
        for name, table, count in mf.slot_tables(n):
            rows = mf.member_counts(n, name)
            np.testing.assert_array_equal(rows.sum(axis=0), c["counts"])
            used = set(np.clip(table, 0, count - 1).tolist())
            assert not rows[[m for m in range(16) if m not in used]].any(), (n, name)
        assert {int(v) for v in mf.slot_tables(n)[2][1]} >= ({-3} if n <= 32 else {-3, 99})
        if n >= 64:
            members, double = mf.coverage(n)
            assert all(v >= 2 for v in members.values()) and double >= 1, (n, members, double)      # every flag under two members; two flags at once
    assert int(mf.case(1)["counts"][0]) == 0                                     # the launch without a done env


def test_learner_win_rate_and_pfsp_weights():
    from legged_games_gym_amd.rl.opponent_pool import learner_win_rate, pfsp_weights
    row = dict(episodes=8, captured=6, timed_out=3, fell=1, ll_timed_out=0, steps=100)      # the flags are not exclusive
    assert learner_win_rate(row, "pred") == 0.75 and learner_win_rate(row, "prey") == 0.25
    assert np.isnan(learner_win_rate(dict(row, episodes=0, captured=0), "pred"))
    with pytest.raises(ValueError):
        learner_win_rate(row, "referee")
    # members: never met, always beaten by the learner, even, always beating the learner
    wins, episodes = [0, 10, 5, 0], [0, 10, 10, 10]
    w = pfsp_weights(wins, episodes, 1.0)
    assert w == [1.0 - 1.0 / 2.0, 1.0 - 11.0 / 12.0, 1.0 - 6.0 / 12.0, 1.0 - 1.0 / 12.0] and w[0] == 0.5      # the unmet member: a rate of 0.5
    assert w[3] > w[2] > w[1] and w[0] == w[2]                                   # monotone: a lower learner win rate, a larger weight
    w2 = pfsp_weights(wins, episodes, 2.0)
    assert w2 == [v ** 2.0 for v in w] and w2[3] / w2[1] > w[3] / w[1]           # a higher power sharpens the deal
    assert pfsp_weights(wins, episodes, 0) == [1.0] * 4 and pfsp_weights([], [], 1.0) == []
    rates = np.linspace(0.0, 1.0, 11)
    ws = pfsp_weights([int(round(100 * r)) for r in rates], [100] * 11, 1.5)
    assert all(a > b for a, b in zip(ws, ws[1:]))
    for bad in (([1], [1, 2], 1.0), ([3], [2], 1.0), ([1], [2], -1.0)):
        with pytest.raises(ValueError):
            pfsp_weights(*bad)


def test_apportion_is_the_largest_remainder_method():
    from legged_games_gym_amd.rl.opponent_pool import apportion
    assert apportion((3, 1), 8) == [6, 2]                                        # one each, then 6 more: quotas 4.5 / 1.5, the tie to the lower index
    assert apportion([1, 1, 1], 31) == [11, 10, 10] and apportion([1, 1, 1], 2) == [1, 1, 0] and apportion([1.0] * 15, 96) == [7] * 6 + [6] * 9
    assert apportion([0.5, 0.5, 0.5, 0.5], 6) == [2, 2, 1, 1] == apportion([0.5, 0.5, 0.5, 0.5], 6)      # ties: deterministic, to the lower index
    assert apportion([0, 0], 5) == [3, 2] and apportion([], 4) == [] and apportion([2.0], 7) == [7] and apportion([1, 2], 0) == [0, 0]
    assert apportion([1e-9, 1.0], 3) == [1, 2] and apportion([0.0, 1.0], 10) == [1, 9]      # at least 1 each when there is enough
    assert apportion([1.0, 5.0, 1.0], 2) == [0, 2, 0]                               # fewer shares than members: by weight alone
    gen = np.random.default_rng(0)
    for _ in range(200):
        k, total = int(gen.integers(1, 16)), int(gen.integers(0, 200))
        weights = gen.random(k) ** 3
        shares = apportion(weights.tolist(), total)
        assert sum(shares) == total and len(shares) == k and min(shares) >= (1 if total >= k else 0)
        rest = total - (k if total >= k else 0)
        quota = rest * weights / weights.sum() + (1 if total >= k else 0)
        assert np.abs(np.array(shares) - quota).max() < 1.0 + 1e-9               # the quota rule
    with pytest.raises(ValueError):
        apportion([1, -1], 3)
    with pytest.raises(ValueError):
        apportion([1, 1], -3)


@pytest.mark.parametrize("blocks,filled,share", [(1, 0, 0.5), (4, 0, 0.5), (63, 3, 0.5), (63, 3, 0.0), (63, 3, 1.0), (128, 15, 0.25)])      # those of test_assign_blocks_counts
def test_assign_blocks_weighted_with_equal_weights_gives_the_counts_of_assign_blocks(blocks, filled, share):
    from legged_games_gym_amd.rl.opponent_pool import assign_blocks, assign_blocks_weighted
    plain = assign_blocks(blocks, filled, share, torch.Generator().manual_seed(7))
    for weight in (1.0, 0.37):
        slots = assign_blocks_weighted(blocks, filled, share, [weight] * filled, torch.Generator().manual_seed(7))
        assert slots.dtype == torch.int32 and slots.shape == (blocks,)
        assert torch.bincount(slots.long(), minlength=filled + 1).tolist() == torch.bincount(plain.long(), minlength=filled + 1).tolist()
        assert torch.equal(slots == 0, plain == 0)                               # the live blocks are drawn exactly as assign_blocks draws them
    if filled == 0:
        assert not slots.any()                                                   # all blocks live


def test_assign_blocks_weighted_cuts_the_permuted_order_into_apportioned_runs():
    from legged_games_gym_amd.rl.opponent_pool import apportion, assign_blocks_weighted
    weights = [0.9, 0.1, 0.5]
    slots = assign_blocks_weighted(63, 3, 0.5, weights, torch.Generator().manual_seed(7))
    perm = torch.randperm(63, generator=torch.Generator().manual_seed(7))
    shares = apportion(weights, 63 - 32)
    assert shares == [18, 3, 10] and torch.bincount(slots.long()).tolist() == [32] + shares
    assert not slots[perm[:32]].any() and slots[perm[32:]].tolist() == [1] * 18 + [2] * 3 + [3] * 10
    assert torch.equal(slots, assign_blocks_weighted(63, 3, 0.5, weights, torch.Generator().manual_seed(7)))
    assert not assign_blocks_weighted(5, 0, 0.5, [], torch.Generator().manual_seed(1)).any()
    with pytest.raises(ValueError):
        assign_blocks_weighted(8, 2, 0.5, [1.0], None)
    with pytest.raises(ValueError):
        assign_blocks_weighted(0, 0, 0.5, [], None)


def test_the_runner_refuses_opponent_priority_without_a_pool_or_the_outcome_statistics():
    """The refusal comes before anything is built, so a stand-in env shows it without a GPU."""
    from legged_games_gym_amd.rl import DecGamePolicyRunner
    from legged_games_gym_amd.rl.dec_runner import opponent_priority_of
    with_stats, without = types.SimpleNamespace(_outcome=object()), types.SimpleNamespace(_outcome=None)
    with pytest.raises(ValueError, match="opponent_pool_size"):
        DecGamePolicyRunner(with_stats, {"runner": {"opponent_priority": 1.0}}, None, "cpu")
    with pytest.raises(ValueError, match="opponent_pool_size"):
        DecGamePolicyRunner(with_stats, {"runner": {"opponent_priority": 1.0, "opponent_pool_size": 0}}, None, "cpu")
    with pytest.raises(ValueError, match="outcome_stats"):
        DecGamePolicyRunner(without, {"runner": {"opponent_priority": 0.5, "opponent_pool_size": 2}}, None, "cpu")
    with pytest.raises(ValueError, match=">= 0"):
        opponent_priority_of({"opponent_priority": -1.0, "opponent_pool_size": 2}, with_stats)
    assert opponent_priority_of({}, without) == 0.0 and opponent_priority_of({"opponent_priority": 0, "opponent_pool_size": 0}, without) == 0.0
    assert opponent_priority_of({"opponent_priority": 2, "opponent_pool_size": 3}, with_stats) == 2.0


def test_the_priority_is_a_flag_and_a_runner_key_but_no_config_field():
    from legged_games_gym_amd.envs.a1_game import DecHighLevelGameCfgPPO
    from legged_games_gym_amd.envs.a1_game.dec_high_level_game import DecHighLevelGame
    from legged_games_gym_amd.rl import OpponentPool
    from legged_games_gym_amd.scripts import train_dec_game
    from legged_games_gym_amd.utils.helpers import class_to_dict
    assert train_dec_game._args([]).opponent_priority == 0.0 and train_dec_game._args(["--opponent_priority", "1.5"]).opponent_priority == 1.5
    assert "opponent_priority" not in class_to_dict(DecHighLevelGameCfgPPO())["runner"]
    assert callable(DecHighLevelGame.enable_member_outcomes)
    for name in ("member_totals_host", "reset_member_totals", "push", "assign", "state", "load_state"):
        assert callable(getattr(OpponentPool, name)), name
