"""The outcome statistics' C-ABI (include/legged_game_outcome.h) without a GPU: the header's functions are ``capi.OUTCOME_SYMBOLS``, the built
library exports them with the ctypes layout and refuses bad arguments before any launch, the two rows of the kernel resource table, the
rates' arithmetic of ``scripts/play_game.py``, and the switch that is a command-line flag and an attribute but no config field."""
import ctypes
import math
import os
import re

import pytest

from legged_games_gym_amd import capi

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
RESOURCES = os.path.join(REPO, "legged_games_gym_amd", "csrc", "kernel_resources.txt")
OTHER = {"legged_hip.h": "EXPORTED_SYMBOLS", "legged_game.h": "GAME_SYMBOLS", "legged_dec_game.h": "DEC_GAME_SYMBOLS", "legged_pursuer_game.h": "PURSUER_SYMBOLS"}
FORBIDDEN = ("k_game_", "k_pursuer_post", "k_prey_act", "k_dec_", "k_step", "k_physics")      # substrings existing tests count rows by


def _declared(header):
    text = open(os.path.join(REPO, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
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


def test_outcome_header_symbol_list_matches_binding_and_is_disjoint_from_the_others():
    assert sorted(_declared("legged_game_outcome.h")) == sorted(capi.OUTCOME_SYMBOLS) == sorted(["lg_outcome_post", "lg_outcome_pursuer_post", "lg_outcome_sizeof"])
    for header, name in OTHER.items():
        assert not set(capi.OUTCOME_SYMBOLS) & set(getattr(capi, name)), name
        assert not set(capi.OUTCOME_SYMBOLS) & set(_declared(header)), header
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "legged_game_outcome.h")).read(), flags=re.S)
    assert "LG_ABI_VERSION" not in text and capi.LG_ABI_VERSION == 22
    assert capi.OUTCOME_COUNTS == ("episodes", "captured", "prey_out", "predator_out", "fell", "survived", "steps")
    assert capi.OUTCOME_MEANS == capi.OUTCOME_COUNTS[1:] and (capi.LG_OUTCOME_NUM_COUNTS, capi.LG_OUTCOME_NUM_MEANS) == (7, 6)
    assert re.search(r"#define\s+LG_OUTCOME_NUM_COUNTS\s+7\b", text) and re.search(r"#define\s+LG_OUTCOME_NUM_MEANS\s+6\b", text)


def test_library_exports_the_outcome_symbols_with_the_ctypes_layout(lib):
    for sym in capi.OUTCOME_SYMBOLS:
        assert hasattr(lib, sym), sym
    lib.lg_outcome_sizeof.argtypes, lib.lg_outcome_sizeof.restype = [ctypes.c_int], ctypes.c_int
    assert lib.lg_outcome_sizeof(0) == ctypes.sizeof(capi.lg_outcome_buffers) == 5 * ctypes.sizeof(ctypes.c_void_p)
    assert lib.lg_outcome_sizeof(1) == -1
    capi.bind_header(lib, "legged_game_outcome.h")                                           # raises on a layout mismatch
    assert [n for n, _ in capi.lg_outcome_buffers._fields_] == ["ll_time_out_buf", "accum", "ticket", "means", "totals"]


def _arguments(num_envs=8):
    """Parameters and pointer tables that pass every check (the addresses are never dereferenced: each call below is refused first)."""
    P = capi.lg_game_params()
    P.num_envs, P.decimation = num_envs, 4
    Q = capi.lg_pursuer_params()
    Q.max_lin_vel, Q.min_lin_vel, Q.gain, Q.max_episode_length = 2.0, 0.01, 2.0, 1000
    B = capi.game_buffers({name: 0x1000 for name in capi.GAME_BUFFER_FIELDS})
    O = capi.outcome_buffers({name: 0x1000 for name in capi.OUTCOME_BUFFER_FIELDS})
    return P, Q, B, O


def test_bad_arguments_are_refused_before_any_launch(lib):
    capi.bind_header(lib, "legged_game_outcome.h")
    r = ctypes.byref
    P, Q, B, O = _arguments()
    # a null struct
    assert lib.lg_outcome_post(None, r(B), r(O), 3, None) == -1
    assert lib.lg_outcome_post(r(P), None, r(O), 3, None) == -1
    assert lib.lg_outcome_post(r(P), r(B), None, 3, None) == -1
    assert lib.lg_outcome_pursuer_post(r(P), None, r(B), r(O), None, 3, None) == -1
    assert lib.lg_outcome_pursuer_post(r(P), r(Q), r(B), None, None, 3, None) == -1
    # a null buffer, of the game's and of the outcome's
    for name in ("ll_root_states", "obs", "reset_buf", "episode_sums"):
        Bn = capi.game_buffers({k: (0 if k == name else 0x1000) for k in capi.GAME_BUFFER_FIELDS})
        assert lib.lg_outcome_post(r(P), r(Bn), r(O), 3, None) == -1, name
        assert lib.lg_outcome_pursuer_post(r(P), r(Q), r(Bn), r(O), None, 3, None) == -1, name
    for name in capi.OUTCOME_BUFFER_FIELDS:
        On = capi.outcome_buffers({k: (0 if k == name else 0x1000) for k in capi.OUTCOME_BUFFER_FIELDS})
        assert lib.lg_outcome_post(r(P), r(B), r(On), 3, None) == -1, name
        assert lib.lg_outcome_pursuer_post(r(P), r(Q), r(B), r(On), None, 3, None) == -1, name
        assert b"lg_outcome_buffers" in lib.lg_last_error()
    # the scripted variant does not read `command`; the plain one does
    Bc = capi.game_buffers({k: (0 if k == "command" else 0x1000) for k in capi.GAME_BUFFER_FIELDS})
    assert lib.lg_outcome_post(r(P), r(Bc), r(O), 3, None) == -1
    # num_envs = 0
    P0, _, _, _ = _arguments(num_envs=0)
    assert lib.lg_outcome_post(r(P0), r(B), r(O), 3, None) == -2 and b"num_envs" in lib.lg_last_error()
    assert lib.lg_outcome_pursuer_post(r(P0), r(Q), r(B), r(O), None, 3, None) == -2 and b"num_envs" in lib.lg_last_error()
    # the pursuer's parameters, the field named
    for field, value in (("max_episode_length", 0), ("max_episode_length", (1 << 20) + 1), ("gain", 0.0), ("max_lin_vel", 0.001)):
        _, Qb, _, _ = _arguments()
        setattr(Qb, field, value)
        assert lib.lg_outcome_pursuer_post(r(P), r(Qb), r(B), r(O), None, 3, None) == -2, (field, value)
        assert field.encode() in lib.lg_last_error(), (field, lib.lg_last_error())
    # the device step counter without its buffer
    Bs = capi.game_buffers({k: (0 if k == "ll_step_counter" else 0x1000) for k in capi.GAME_BUFFER_FIELDS})
    assert lib.lg_outcome_post(r(P), r(Bs), r(O), -1, None) == -9
    assert lib.lg_outcome_pursuer_post(r(P), r(Q), r(Bs), r(O), None, -1, None) == -9


def test_kernel_resource_table_lists_the_two_outcome_kernels():
    lines = [l for l in open(RESOURCES) if not l.startswith("#") and "k_outcome_post" in l]
    assert len(lines) == 2 and any("ILb0E" in l for l in lines) and any("ILb1E" in l for l in lines), lines
    for line in lines:
        assert " spill 0 " in line and " scratch 0 " in line and " AGPRs 0 " in line, line
        lds = int(re.search(r"LDS (\d+)", line).group(1))
        assert 0 < lds <= 7 * 4 * 8, line
        for sub in FORBIDDEN:
            assert sub not in line.split()[0], (sub, line)


def test_outcome_rates_on_hand_made_totals():
    from legged_games_gym_amd.scripts.play_game import COUNTS, outcome_rates
    assert COUNTS == capi.OUTCOME_COUNTS
    got = outcome_rates(dict(episodes=8, captured=4, prey_out=1, predator_out=0, fell=2, survived=3, steps=1000))
    assert got == dict(captured_rate=0.5, prey_out_rate=0.125, predator_out_rate=0.0, fell_rate=0.25, survived_rate=0.375, mean_steps=125.0)
    assert sum(got[k] for k in got if k.endswith("_rate")) > 1.0                          # the flags are not exclusive
    one = outcome_rates(dict(episodes=1, captured=1, prey_out=0, predator_out=0, fell=0, survived=0, steps=(1 << 40) + 1))
    assert one["captured_rate"] == 1.0 and one["mean_steps"] == float((1 << 40) + 1)
    none = outcome_rates(dict(episodes=0, captured=0, prey_out=0, predator_out=0, fell=0, survived=0, steps=0))
    assert set(none) == set(got) and all(math.isnan(v) for v in none.values())


def test_the_switch_is_a_flag_and_an_attribute_but_no_config_field():
    from legged_games_gym_amd.envs.a1_game import HighLevelGameFlatCfg, ScriptedPredatorGameCfg
    from legged_games_gym_amd.utils import get_args
    from legged_games_gym_amd.utils.helpers import class_to_dict
    for cls in (HighLevelGameFlatCfg, ScriptedPredatorGameCfg):
        d = class_to_dict(cls())
        assert "outcome_stats" not in d["env"] and "outcome_stats" not in d
        assert getattr(cls().env, "outcome_stats", False) is False
    assert get_args([]).outcome_stats is False
    assert get_args(["--outcome_stats"]).outcome_stats is True


def test_the_registered_game_configs_carry_no_switch():
    from legged_games_gym_amd.envs import a1_game, task_registry
    from legged_games_gym_amd.utils.helpers import class_to_dict
    a1_game.register()
    a1_game.register_scripted()
    try:
        for name in ("high_level_game", "scripted_predator_game"):
            env_cfg, train_cfg = task_registry.get_cfgs(name)
            assert "outcome_stats" not in class_to_dict(env_cfg)["env"] and "outcome_stats" not in class_to_dict(train_cfg)["runner"], name
    finally:
        a1_game.unregister()
        a1_game.unregister_scripted()


def test_the_seeded_device_cases_cover_every_flag_on_the_twin():
    """The inputs tests/test_gpu_outcome.py sends to the device, checked on the twin alone: over the parametrisation every flag occurs, some
    env raises two at once and every done env raises one; the four-call sequence has its quiet call and stays clear of the capture threshold."""
    from tests import outcome_fixtures as of
    occurs, double, bare = of.coverage()
    assert all(v > 0 for v in occurs.values()), occurs
    assert double > 0 and bare == 0
    for scripted in (False, True):
        rows = of.sequence_twin(scripted)
        assert [int(c[0]) > 0 for c, _ in rows] == [k != of.SEQ_QUIET for k in range(of.SEQ_CALLS)]
        assert min(m for _, m in rows) >= 1e-4


def test_twin_on_a_hand_made_step():
    import numpy as np
    from tests import outcome_twin as ot
    p = dict(capture_dist=0.5, env_radius=3.0)
    dn = dict(dist_xy=np.array([0.4, 2.0, 2.0, 0.1, 2.0], np.float32), prey_r=np.array([1.0, 4.0, 1.0, 3.5, 1.0], np.float32),
              pred_r=np.array([1.0, 1.0, 1.0, 1.0, 1.0], np.float32))
    f, c, m = ot.outcome(p, dn, ll_reset=[0, 0, 1, 1, 0], ll_time_out=[0, 0, 1, 0, 0], curr_episode_step=np.array([9, 19, 29, 39, 49]))
    assert f["done"].tolist() == [True, True, True, True, False]
    assert c.tolist() == [4, 2, 2, 0, 1, 1, 10 + 20 + 30 + 40]             # env 3 is captured, outside and fallen at once
    assert m.tolist() == [0.5, 0.5, 0.0, 0.25, 0.25, 25.0] and m.dtype == np.float32
    _, c0, m0 = ot.outcome(dict(p, env_radius=-1.0), dict(dn, dist_xy=dn["dist_xy"] + 1), [0] * 5, [0] * 5, np.zeros(5, np.int64), previous_means=m)
    assert c0.tolist() == [0] * 7 and m0.tolist() == m.tolist()
