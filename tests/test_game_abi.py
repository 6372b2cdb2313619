"""The game layer's C-ABI (include/legged_game.h): the header's functions are ``capi.GAME_SYMBOLS``, the built library exports them with the
ctypes layouts, the locomotion ABI is untouched, and importing the game package registers nothing."""
import ctypes
import os
import re

from legged_games_gym_amd import capi
from tests.game_fixtures import LOCOMOTION_TASKS, game_registered  # noqa: F401

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))


def _declared(header):
    text = open(os.path.join(REPO, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.findall(r"\b(lg_[a-z_0-9]+)\s*\(", text)


def test_game_header_symbol_list_matches_binding():
    assert sorted(_declared("legged_game.h")) == sorted(capi.GAME_SYMBOLS)
    assert not set(capi.GAME_SYMBOLS) & set(capi.EXPORTED_SYMBOLS)
    assert not set(_declared("legged_hip.h")) & set(capi.GAME_SYMBOLS)          # the locomotion header does not know the game


def test_library_exports_the_game_symbols_with_the_ctypes_layouts():
    path = capi.library_path()
    if not os.path.isfile(path):
        import __graft_entry__ as entry
        entry.build()
    lib = ctypes.CDLL(path)
    for sym in capi.GAME_SYMBOLS:
        assert hasattr(lib, sym), sym
    lib.lg_game_sizeof.argtypes, lib.lg_game_sizeof.restype = [ctypes.c_int], ctypes.c_int
    assert lib.lg_game_sizeof(0) == ctypes.sizeof(capi.lg_game_params)
    assert lib.lg_game_sizeof(1) == ctypes.sizeof(capi.lg_game_buffers)
    assert lib.lg_game_sizeof(2) == -1
    capi.bind_header(lib, "legged_game.h")                                              # raises on a layout mismatch
    assert ctypes.sizeof(capi.lg_game_params) % 8 == 0 and capi.lg_game_params.seed.offset % 8 == 0
    assert capi.lg_game_params.base_init_state.size == 13 * 4


def test_locomotion_abi_is_unchanged():
    text = open(os.path.join(REPO, "include", "legged_hip.h")).read()
    assert capi.LG_ABI_VERSION == 22 and re.search(r"#define\s+LG_ABI_VERSION\s+22\b", text)
    assert "LG_ABI_VERSION" not in re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "legged_game.h")).read(), flags=re.S)


def test_kernel_resource_table_lists_the_two_game_kernels():
    rows = [l.split()[0] for l in open(os.path.join(REPO, "legged_games_gym_amd", "csrc", "kernel_resources.txt")) if not l.startswith("#")]
    game = [r for r in rows if "k_game_" in r]
    assert len(game) == 2 and any("k_game_pre" in r for r in game) and any("k_game_post" in r for r in game)
    for line in open(os.path.join(REPO, "legged_games_gym_amd", "csrc", "kernel_resources.txt")):
        if "k_game_" in line:
            assert "spill 0" in line and "scratch 0" in line and "LDS 0" in line, line


def test_import_registers_nothing_and_register_adds_the_task():
    import legged_games_gym_amd.envs.a1_game as a1_game
    from legged_games_gym_amd.envs import task_registry
    assert a1_game.TASKS == ("high_level_game",)
    assert set(task_registry.task_classes) == LOCOMOTION_TASKS


def test_register_and_restore(game_registered):
    from legged_games_gym_amd.envs.a1_game import HighLevelGame, HighLevelGameFlatCfg, HighLevelGameFlatCfgPPO
    reg = game_registered
    assert set(reg.task_classes) == LOCOMOTION_TASKS | {"high_level_game"} and len(reg.task_classes) == 6
    assert reg.get_task_class("high_level_game") is HighLevelGame
    env_cfg, train_cfg = reg.get_cfgs("high_level_game")
    assert isinstance(env_cfg, HighLevelGameFlatCfg) and isinstance(train_cfg, HighLevelGameFlatCfgPPO)
    assert env_cfg.seed == train_cfg.seed == 1 and train_cfg.runner.experiment_name == "high_level_game_flat"
    assert not hasattr(HighLevelGame, "_sim")                   # what selects the runner's generic VecEnv path


def test_registry_is_back_to_five_after_the_fixture():
    from legged_games_gym_amd.envs import task_registry
    assert set(task_registry.task_classes) == LOCOMOTION_TASKS
