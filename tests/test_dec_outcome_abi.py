"""The decentralised game's outcome statistics without a GPU: the header's functions are ``capi.DEC_OUTCOME_SYMBOLS`` (include/
legged_dec_game_outcome.h), the built library exports them with the ctypes layout and refuses bad arguments before any launch, the row of the
kernel resource table, the NumPy twin (tests/dec_outcome_twin.py) on a hand-made step and on the seeded cases the device tests use, the
rates' arithmetic of ``scripts/play_dec_game.py``, and the switch that is a command-line flag and an attribute but no config field."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from legged_games_gym_amd import capi

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
RESOURCES = os.path.join(REPO, "legged_games_gym_amd", "csrc", "kernel_resources.txt")
HEADER = "legged_dec_game_outcome.h"
OTHER = {"legged_hip.h": "EXPORTED_SYMBOLS", "legged_game.h": "GAME_SYMBOLS", "legged_dec_game.h": "DEC_GAME_SYMBOLS", "legged_pursuer_game.h": "PURSUER_SYMBOLS",
         "legged_game_outcome.h": "OUTCOME_SYMBOLS"}
FORBIDDEN = ("k_dec_post", "k_outcome_post", "k_dec_pre", "k_dec_act", "k_game_", "k_pursuer_post", "k_prey_act", "k_step", "k_physics")      # substrings existing tests count rows by


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
    assert sorted(_declared(HEADER)) == sorted(capi.DEC_OUTCOME_SYMBOLS) == sorted(["lg_dec_outcome_post", "lg_dec_outcome_sizeof"])
    for header, name in OTHER.items():
        assert not set(capi.DEC_OUTCOME_SYMBOLS) & set(getattr(capi, name)), name
        assert not set(capi.DEC_OUTCOME_SYMBOLS) & set(_declared(header)), header
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", HEADER)).read(), flags=re.S)
    assert "LG_ABI_VERSION" not in text and capi.LG_ABI_VERSION == 22
    assert re.search(r"#define\s+LG_ABI_VERSION\s+22\b", open(os.path.join(REPO, "include", "legged_hip.h")).read())
    assert capi.DEC_OUTCOME_COUNTS == ("episodes", "captured", "timed_out", "fell", "ll_timed_out", "steps")
    assert capi.DEC_OUTCOME_MEANS == capi.DEC_OUTCOME_COUNTS[1:] and (capi.LG_DEC_OUTCOME_NUM_COUNTS, capi.LG_DEC_OUTCOME_NUM_MEANS) == (6, 5)
    assert re.search(r"#define\s+LG_DEC_OUTCOME_NUM_COUNTS\s+6\b", text) and re.search(r"#define\s+LG_DEC_OUTCOME_NUM_MEANS\s+5\b", text)


def test_library_exports_the_symbols_with_the_ctypes_layout(lib):
    for sym in capi.DEC_OUTCOME_SYMBOLS:
        assert hasattr(lib, sym), sym
    lib.lg_dec_outcome_sizeof.argtypes, lib.lg_dec_outcome_sizeof.restype = [ctypes.c_int], ctypes.c_int
    assert lib.lg_dec_outcome_sizeof(0) == ctypes.sizeof(capi.lg_dec_outcome_buffers) == 4 * ctypes.sizeof(ctypes.c_void_p)
    assert lib.lg_dec_outcome_sizeof(1) == -1
    capi.bind_header(lib, "legged_dec_game_outcome.h")                                       # raises on a layout mismatch
    assert capi.DEC_OUTCOME_BUFFER_FIELDS == ["ll_time_out_buf", "accum", "means", "totals"]      # no ticket: the launch draws lg_dec_game_buffers.extras_ticket
    lib.lg_abi_version.restype = ctypes.c_int
    assert lib.lg_abi_version() == 22


def _arguments(num_envs=8):
    """Parameters and pointer tables that pass every check (the addresses are never dereferenced: each call below is refused first)."""
    P = capi.lg_dec_game_params()
    P.num_envs, P.decimation, P.max_episode_length_s = num_envs, 4, 20.0
    B = capi.dec_game_buffers({name: 0x1000 for name in capi.DEC_GAME_BUFFER_FIELDS})
    O = capi.dec_outcome_buffers({name: 0x1000 for name in capi.DEC_OUTCOME_BUFFER_FIELDS})
    return P, B, O


def test_bad_arguments_are_refused_before_any_launch(lib):
    capi.bind_header(lib, "legged_dec_game_outcome.h")
    r = ctypes.byref
    P, B, O = _arguments()
    # a null struct; the outcome's is named
    assert lib.lg_dec_outcome_post(None, r(B), r(O), 3, None) == -1
    assert lib.lg_dec_outcome_post(r(P), None, r(O), 3, None) == -1
    assert lib.lg_dec_outcome_post(r(P), r(B), None, 3, None) == -1 and b"lg_dec_outcome_buffers" in lib.lg_last_error()
    # a null buffer, of the game's and of the outcome's
    for name in ("ll_root_states", "ll_dof_state", "obs_prey", "reset_buf", "episode_sums", "episode_means", "extras_accum", "extras_ticket", "command_pred"):
        Bn = capi.dec_game_buffers({k: (0 if k == name else 0x1000) for k in capi.DEC_GAME_BUFFER_FIELDS})
        assert lib.lg_dec_outcome_post(r(P), r(Bn), r(O), 3, None) == -1, name
    for name in capi.DEC_OUTCOME_BUFFER_FIELDS:
        On = capi.dec_outcome_buffers({k: (0 if k == name else 0x1000) for k in capi.DEC_OUTCOME_BUFFER_FIELDS})
        assert lib.lg_dec_outcome_post(r(P), r(B), r(On), 3, None) == -1, name
        assert b"lg_dec_outcome_buffers" in lib.lg_last_error()
    # what the post stage does not read may be null: the prey's command and the low-level commands
    # (not launched: the next check refuses it)
    P0, _, _ = _arguments(num_envs=0)
    assert lib.lg_dec_outcome_post(r(P0), r(B), r(O), 3, None) == -2 and b"num_envs" in lib.lg_last_error()
    Pz, _, _ = _arguments()
    Pz.max_episode_length_s = 0.0
    assert lib.lg_dec_outcome_post(r(Pz), r(B), r(O), 3, None) == -2 and b"max_episode_length_s" in lib.lg_last_error()
    # the device step counter without its buffer
    Bs = capi.dec_game_buffers({k: (0 if k == "ll_step_counter" else 0x1000) for k in capi.DEC_GAME_BUFFER_FIELDS})
    assert lib.lg_dec_outcome_post(r(P), r(Bs), r(O), -1, None) == -9
    # the plain entry point keeps its codes and its text
    capi.bind_header(lib, "legged_dec_game.h")
    assert lib.lg_dec_game_post(r(P), r(Bs), -1, None) == -9
    Bn = capi.dec_game_buffers({k: (0 if k == "obs_pred" else 0x1000) for k in capi.DEC_GAME_BUFFER_FIELDS})
    assert lib.lg_dec_game_post(r(P), r(Bn), 3, None) == -1 and b"lg_dec_game_post: a buffer pointer is null" in lib.lg_last_error()


def test_kernel_resource_table_lists_the_outcome_kernel_and_keeps_the_plain_one():
    rows = [l for l in open(RESOURCES) if not l.startswith("#")]
    mine = [l for l in rows if "k_dec_outcome" in l]
    assert len(mine) == 1, mine
    f = dict(zip(mine[0].split()[1::2], map(int, mine[0].split()[2::2])))
    assert f["occupancy"] == 8 and f["VGPRs"] <= 64 and f["spill"] == 0 and f["scratch"] == 0 and f["AGPRs"] == 0, mine[0]
    assert 0 < f["LDS"] <= 4 * (6 * 8 + 4 * 4), mine[0]                           # six 64-bit integers and four floats per wave, four waves
    for sub in FORBIDDEN:
        assert sub not in mine[0].split()[0], (sub, mine[0])
    plain = [l for l in rows if "k_dec_post" in l]
    assert len(plain) == 1
    g = dict(zip(plain[0].split()[1::2], map(int, plain[0].split()[2::2])))
    assert g["occupancy"] == 8 and g["VGPRs"] <= 64 and g["LDS"] <= 64 and g["spill"] == 0 and g["scratch"] == 0 and g["AGPRs"] == 0, plain[0]


def test_outcome_rates_on_hand_made_totals():
    from legged_games_gym_amd.scripts.play_dec_game import COUNTS, FLAGS, dec_outcome_rates
    assert COUNTS == capi.DEC_OUTCOME_COUNTS and FLAGS == COUNTS[1:5]
    got = dec_outcome_rates(dict(episodes=8, captured=4, timed_out=1, fell=2, ll_timed_out=3, steps=1000))
    assert got == dict(captured_rate=0.5, timed_out_rate=0.125, fell_rate=0.25, ll_timed_out_rate=0.375, mean_steps=125.0)
    assert sum(got[k] for k in got if k.endswith("_rate")) > 1.0                          # the flags are not exclusive
    one = dec_outcome_rates(dict(episodes=1, captured=1, timed_out=0, fell=0, ll_timed_out=0, steps=(1 << 40) + 1))
    assert one["captured_rate"] == 1.0 and one["mean_steps"] == float((1 << 40) + 1)
    none = dec_outcome_rates(dict(episodes=0, captured=0, timed_out=0, fell=0, ll_timed_out=0, steps=0))
    assert set(none) == set(got) and all(math.isnan(v) for v in none.values())


def test_the_switch_is_a_flag_and_an_attribute_but_no_config_field():
    from legged_games_gym_amd.envs import a1_game, task_registry
    from legged_games_gym_amd.envs.a1_game import DecHighLevelGameCfg, DecHighLevelGameCfgPPO
    from legged_games_gym_amd.envs.a1_game.dec_high_level_game import DecHighLevelGame
    from legged_games_gym_amd.scripts import train_dec_game
    from legged_games_gym_amd.utils.helpers import class_to_dict
    d = class_to_dict(DecHighLevelGameCfg())
    assert "outcome_stats" not in d["env"] and "outcome_stats" not in d and "outcome_stats" not in class_to_dict(DecHighLevelGameCfgPPO())["runner"]
    assert getattr(DecHighLevelGameCfg().env, "outcome_stats", False) is False
    assert train_dec_game._args([]).outcome_stats is False and train_dec_game._args(["--outcome_stats"]).outcome_stats is True
    for name in ("enable_outcome_stats", "outcome_totals", "reset_outcome_totals", "_post"):
        assert callable(getattr(DecHighLevelGame, name)), name
    a1_game.register_dec()
    try:
        env_cfg, train_cfg = task_registry.get_cfgs("dec_high_level_game")
        assert "outcome_stats" not in class_to_dict(env_cfg)["env"] and "outcome_stats" not in class_to_dict(train_cfg)["runner"]
    finally:
        a1_game.unregister_dec()


def test_the_seeded_device_cases_cover_every_flag_on_the_twin():
    """The inputs tests/test_gpu_dec_outcome.py sends to the device, checked on the twin alone: over the 18 cases every flag occurs, some env
    raises two at once, every done env raises one and no other env any; the n = 1 cases have no done env and the forced one exactly one; the
    four-call sequence has its quiet call and stays clear of the capture threshold."""
    from tests import dec_outcome_fixtures as of
    occurs, double, bare, margin = of.coverage()
    assert occurs == dict(captured=1403, timed_out=819, fell=720, ll_timed_out=694) and double == 337 and bare == 0 and margin > 2e-4
    assert all(int(of.case(1, t)["counts"][0]) == 0 for t in of.TERMINATIONS)
    one = of.single_done_case()
    assert one["counts"].tolist()[:5] == [1, 0, 0, 1, 0] and int(one["counts"][5]) == int(one["s"]["curr_episode_step"][0]) + 1
    rows = of.sequence_twin()
    assert [int(c[0]) > 0 for c, _ in rows] == [k != of.SEQ_QUIET for k in range(of.SEQ_CALLS)]
    assert min(m for _, m in rows) >= 1e-4
    total = sum(c for c, _ in rows)
    assert all(int(v) > 0 for v in total), total.tolist()                             # every flag occurs in the sequence as well


def test_twin_on_a_hand_made_step():
    from tests import dec_outcome_twin as ot
    info = dict(capture=np.array([1, 0, 0, 1, 0], bool), time_out=np.array([0, 1, 0, 1, 0], bool), done=np.array([1, 1, 1, 1, 0], bool))
    f, c, m = ot.outcome(info, ll_reset=[0, 0, 1, 1, 0], ll_time_out=[0, 0, 1, 0, 0], curr_episode_step=np.array([9, 19, 29, 39, 49]))
    assert f["done"].tolist() == [True, True, True, True, False]
    assert c.tolist() == [4, 2, 2, 1, 1, 10 + 20 + 30 + 40]                 # env 3 is captured, timed out and fallen at once
    assert m.tolist() == [0.5, 0.5, 0.25, 0.25, 25.0] and m.dtype == np.float32
    quiet = dict(capture=np.zeros(5, bool), time_out=np.zeros(5, bool), done=np.zeros(5, bool))
    _, c0, m0 = ot.outcome(quiet, [0] * 5, [0] * 5, np.zeros(5, np.int64), previous_means=m)
    assert c0.tolist() == [0] * 6 and m0.tolist() == m.tolist()
    with pytest.raises(AssertionError):                                     # a done env without a cause is not a state of the game
        ot.outcome(dict(quiet, done=np.array([1, 0, 0, 0, 0], bool)), [0] * 5, [0] * 5, np.zeros(5, np.int64))
