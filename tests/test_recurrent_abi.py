"""The LSTM cell's C-ABI without a GPU: the header's functions are ``capi.RECURRENT_SYMBOLS`` (include/legged_recurrent.h), the built
library exports them and refuses bad arguments before any launch or allocation, and the rows of the kernel resource table."""
import ctypes
import os
import re

import pytest

from legged_games_gym_amd import capi

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
RESOURCES = os.path.join(REPO, "legged_games_gym_amd", "csrc", "kernel_resources.txt")
HEADER = "legged_recurrent.h"
OTHER = {"legged_hip.h": "EXPORTED_SYMBOLS", "legged_game.h": "GAME_SYMBOLS", "legged_dec_game.h": "DEC_GAME_SYMBOLS", "legged_pursuer_game.h": "PURSUER_SYMBOLS",
         "legged_game_outcome.h": "OUTCOME_SYMBOLS", "legged_dec_game_outcome.h": "DEC_OUTCOME_SYMBOLS", "legged_dec_game_pool.h": "DEC_POOL_SYMBOLS",
         "legged_dec_game_member_outcome.h": "DEC_MEMBER_OUTCOME_SYMBOLS"}
FORBIDDEN = ("k_step", "k_physics", "k_policy_act", "k_prey_act", "k_pool_act", "k_dec_", "k_game_", "k_outcome_post", "k_pursuer_post", "k_member_outcome")


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
    return capi.bind_header(lib, "legged_recurrent.h")


def test_header_symbol_list_matches_binding_and_is_disjoint_from_the_others():
    assert sorted(_declared(HEADER)) == sorted(capi.RECURRENT_SYMBOLS)
    assert {"lg_lstm_create", "lg_lstm_load_device", "lg_lstm_destroy", "lg_lstm_step"} <= set(capi.RECURRENT_SYMBOLS)
    assert set(capi.RECURRENT_SYMBOLS) - {"lg_lstm_create", "lg_lstm_load_device", "lg_lstm_destroy", "lg_lstm_step"} == {
        "lg_lstm_actor_create", "lg_lstm_actor_load_device", "lg_lstm_actor_destroy", "lg_lstm_actor_act"}
    for header, name in OTHER.items():
        assert not set(capi.RECURRENT_SYMBOLS) & set(getattr(capi, name)), name
        assert not set(capi.RECURRENT_SYMBOLS) & set(_declared(header)), header
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", HEADER)).read(), flags=re.S)
    assert "LG_ABI_VERSION" not in text and capi.LG_ABI_VERSION == 22
    assert re.search(r"#define\s+LG_LSTM_MAX_IN\s+256\b", text) and capi.LG_LSTM_MAX_IN == 256
    assert re.search(r"#define\s+LG_LSTM_MAX_HIDDEN\s+256\b", text) and capi.LG_LSTM_MAX_HIDDEN == 256
    assert re.search(r"#define\s+LG_LSTM_BLOCK_ENVS\s+32\b", text) and capi.LG_LSTM_BLOCK_ENVS == 32


def test_library_exports_the_symbols(lib):
    for sym in capi.RECURRENT_SYMBOLS:
        assert hasattr(lib, sym), sym
    assert len(lib.lg_lstm_step.argtypes) == 15 and len(lib.lg_lstm_create.argtypes) == 8
    lib.lg_abi_version.restype = ctypes.c_int
    assert lib.lg_abi_version() == 22
    import __graft_entry__ as entry
    assert "lg_recurrent.hip" in entry.HIP_SOURCES and "lg_recurrent.h" in entry.HIP_HEADERS
    assert any(h.endswith(os.path.join("include", HEADER)) for h in entry.HIP_HEADERS)


def _step(lib, la=0x1000, lc=0x1000, num_envs=8, h_out_a=0x3000, c_out_a=0x4000, h_in_a=0x1000, c_in_a=0x2000, x_a=0x5000):
    """``lg_lstm_step`` on addresses that are never dereferenced: every call below is refused first."""
    return lib.lg_lstm_step(la, lc, x_a, 0x5000, None, h_in_a, c_in_a, h_out_a, c_out_a, 0x6000, 0x7000, 0x8000, 0x9000, num_envs, None)


def test_bad_arguments_are_refused_before_any_launch_or_allocation(lib):
    out = ctypes.c_void_p()
    w = 0x1000                                               # never dereferenced: the shape is checked first
    assert lib.lg_lstm_create(48, 64, w, w, w, w, 0, None) == -1
    assert lib.lg_lstm_create(48, 64, None, w, w, w, 0, ctypes.byref(out)) == -1
    for hidden in (48, 288, 0, 16):
        assert lib.lg_lstm_create(48, hidden, w, w, w, w, 0, ctypes.byref(out)) == -4 and b"hidden" in lib.lg_last_error(), hidden
    for num_in in (0, 257, -1):
        assert lib.lg_lstm_create(num_in, 64, w, w, w, w, 0, ctypes.byref(out)) == -4 and b"num_in" in lib.lg_last_error(), num_in
    assert not out.value
    assert lib.lg_lstm_destroy(None) == -1
    assert lib.lg_lstm_load_device(None, w, w, w, w, None) == -1 and lib.lg_lstm_load_device(w, w, None, w, w, None) == -1
    assert _step(lib, la=None, lc=None) == -1 and b"both" in lib.lg_last_error()
    assert _step(lib, x_a=None) == -1 and _step(lib, h_out_a=None) == -1
    for n in (0, -5):
        assert _step(lib, num_envs=n) == -2 and b"num_envs" in lib.lg_last_error(), n
    assert _step(lib, h_out_a=0x1000) == -2 and b"alias" in lib.lg_last_error()          # h_out == h_in
    assert _step(lib, c_out_a=0x2000) == -2 and _step(lib, lc=None, h_out_a=0x2000) == -2
    # the actor MLP behind the memory
    dims = lambda *d: (ctypes.c_int32 * 5)(*d)
    assert lib.lg_lstm_actor_create(None, 0, ctypes.byref(out)) == -1 and lib.lg_lstm_actor_create(dims(64, 128, 64, 32, 12), 0, None) == -1
    for bad in ((48, 128, 64, 32, 12), (288, 128, 64, 32, 12), (64, 120, 64, 32, 12), (64, 128, 64, 544, 12), (64, 128, 64, 32, 0), (64, 128, 64, 32, 17)):
        assert lib.lg_lstm_actor_create(dims(*bad), 0, ctypes.byref(out)) == -4, bad
    assert not out.value
    assert lib.lg_lstm_actor_destroy(None) == -1 and lib.lg_lstm_actor_load_device(None, None, None, None, None) == -1
    assert lib.lg_lstm_actor_act(None, w, w, w, 8, 1, 1, None, 0, None) == -1 and lib.lg_lstm_actor_act(w, None, w, w, 8, 1, 1, None, 0, None) == -1
    assert lib.lg_lstm_actor_act(w, w, w, w, 0, 1, 1, None, 0, None) == -2
    assert capi.lstm_supported(48, 256) and capi.lstm_supported(1, 32) and capi.lstm_supported(256, 256)
    assert not capi.lstm_supported(48, 512) and not capi.lstm_supported(48, 48) and not capi.lstm_supported(257, 64) and not capi.lstm_supported(0, 64)


def test_kernel_resource_table_lists_the_cell_and_keeps_the_others():
    rows = [l for l in open(RESOURCES) if not l.startswith("#")]
    fields = lambda row: dict(zip(row.split()[1::2], map(int, row.split()[2::2])))
    learner = open(os.path.join(REPO, "tests", "test_learner_kernel_coverage.py")).read()
    for kernel in ("k_lstm_cell", "k_lstm_pack", "k_lstm_actor", "k_lstm_actor_pack"):
        mine = [l for l in rows if kernel + "E" in l.split()[0]]              # (the mangled name ends the identifier with E)
        assert len(mine) == 1, mine
        f = fields(mine[0])
        assert f["spill"] == 0 and f["scratch"] == 0, mine[0]
        for sub in FORBIDDEN:
            assert sub not in mine[0].split()[0], (sub, mine[0])
        assert kernel not in learner                          # none of the learner kernel names that file lists
    assert len([l for l in rows if "k_step" in l or "k_physics" in l]) == 32
