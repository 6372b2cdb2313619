"""The decentralised game's C-ABI (include/legged_dec_game.h), config, fixtures' provenance and registration, without a GPU: the header's
functions are ``capi.DEC_GAME_SYMBOLS``, the built library exports them with the ctypes layouts, the resource table lists the new kernels
without spills, the config classes equal the reference's own value for value, and importing the package registers nothing."""
import ctypes
import hashlib
import json
import os
import re

import pytest

from legged_games_gym_amd import capi
from legged_games_gym_amd.utils.helpers import class_to_dict
from tests.dec_game_fixtures import dec_registered  # noqa: F401
from tests.game_fixtures import LOCOMOTION_TASKS
from tests.test_golden_provenance import REF            # where the reference tree lies when it is present (build container only)

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
RESOURCES = os.path.join(REPO, "legged_games_gym_amd", "csrc", "kernel_resources.txt")
NEW_FIELDS = {("env", "ll_policy_path"): None}        # fields this build adds to the reference's config, with their defaults


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", header)).read(), flags=re.S)
    return re.findall(r"\b(lg_[a-z_0-9]+)\s*\(", text)


def _rows():
    return {l.split()[0]: l.rstrip("\n") for l in open(RESOURCES) if not l.startswith("#")}


def test_header_symbol_list_matches_binding():
    assert sorted(_declared("legged_dec_game.h")) == sorted(capi.DEC_GAME_SYMBOLS)
    assert not set(capi.DEC_GAME_SYMBOLS) & (set(capi.GAME_SYMBOLS) | set(capi.EXPORTED_SYMBOLS))
    assert not (set(_declared("legged_hip.h")) | set(_declared("legged_game.h"))) & set(capi.DEC_GAME_SYMBOLS)


def test_library_exports_the_symbols_with_the_ctypes_layouts():
    path = capi.library_path()
    if not os.path.isfile(path):
        import __graft_entry__ as entry
        entry.build()
    lib = ctypes.CDLL(path)
    for sym in capi.DEC_GAME_SYMBOLS:
        assert hasattr(lib, sym), sym
    lib.lg_dec_game_sizeof.argtypes, lib.lg_dec_game_sizeof.restype = [ctypes.c_int], ctypes.c_int
    assert lib.lg_dec_game_sizeof(0) == ctypes.sizeof(capi.lg_dec_game_params)
    assert lib.lg_dec_game_sizeof(1) == ctypes.sizeof(capi.lg_dec_game_buffers)
    assert lib.lg_dec_game_sizeof(2) == ctypes.sizeof(capi.lg_dec_act_outputs)
    assert lib.lg_dec_game_sizeof(3) == -1
    capi.bind_header(lib, "legged_dec_game.h")                                          # raises on a layout mismatch
    assert ctypes.sizeof(capi.lg_dec_game_params) % 8 == 0 and capi.lg_dec_game_params.seed.offset % 8 == 0
    assert capi.lg_dec_game_params.base_init_state.size == 13 * 4 and capi.lg_dec_game_params.default_dof_pos.size == 12 * 4
    decl = re.search(r"\bint\s+lg_dec_game_act\s*\((.*?)\)\s*;", re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "legged_dec_game.h")).read(), flags=re.S),
                     flags=re.S).group(1)
    assert len(decl.split(",")) == len(lib.lg_dec_game_act.argtypes) == 20
    # null arguments are refused before anything is launched (no GPU needed)
    assert lib.lg_dec_game_pre(None, None, None) == -1 and lib.lg_dec_game_post(None, None, 0, None) == -1
    lib.lg_last_error.restype = ctypes.c_char_p
    assert b"null" in lib.lg_last_error()


def test_resource_table_lists_the_new_kernels_without_spills():
    rows = _rows()
    pre = [r for n, r in rows.items() if "k_dec_pre" in n]
    post = [r for n, r in rows.items() if "k_dec_post" in n]
    act = [r for n, r in rows.items() if "k_dec_act" in n]
    f32 = [r for n, r in rows.items() if "k_policy_actILi1ELi32ELi16ELi8E" in n]
    wide = [r for n, r in rows.items() if "k_policy_act_wideILi1ELi16ELi8ELi4E" in n]
    assert [len(x) for x in (pre, post, act, f32, wide)] == [1] * 5
    for r in pre + post + act + f32 + wide:
        assert "spill 0" in r and "scratch 0" in r, r
        assert "k_game_" not in r and "k_prey_act" not in r                      # the counts of tests/test_game_abi.py / test_game_policy_abi.py
    assert "LDS 0" in pre[0]
    assert int(re.search(r"LDS (\d+)", post[0]).group(1)) <= 4 * 4 * 4            # the extras reduction: 4 values x 4 waves
    wide_lds = max(int(re.search(r"LDS (\d+)", r).group(1)) for n, r in rows.items() if "k_policy_act_wide" in n)
    assert int(re.search(r"LDS (\d+)", act[0]).group(1)) <= wide_lds <= 98304
    assert sum(("k_step" in n or "k_physics" in n) for n in rows) == 32          # the step kernels are the parent's


def test_config_values_match_reference(golden_dir):
    from legged_games_gym_amd.envs.a1_game import DecHighLevelGameCfg, DecHighLevelGameCfgPPO
    norm = lambda x: json.loads(json.dumps(x))
    gold = json.load(open(os.path.join(golden_dir, "dec_game_configs.json")))["dec_high_level_game"]
    env, train = norm(class_to_dict(DecHighLevelGameCfg())), norm(class_to_dict(DecHighLevelGameCfgPPO()))
    for (section, key), default in NEW_FIELDS.items():
        assert key not in gold["env"][section]
        assert env[section].pop(key) == default
    assert env == gold["env"]                       # key for key
    assert train == gold["train"]
    assert (env["env"]["num_observations_prey"], env["env"]["num_actions_prey"], env["env"]["num_observations_predator"], env["env"]["num_actions_predator"]) == (16, 4, 3, 2)
    assert train["runner"]["max_iterations"] == 200 and train["runner"]["max_evolutions"] == 20
    a, b = DecHighLevelGameCfg(), DecHighLevelGameCfg()
    a.env.num_envs = 7
    assert b.env.num_envs == 2000 and DecHighLevelGameCfg.env.num_envs == 2000


def test_provenance_lists_the_fixtures(golden_dir):
    table = json.load(open(os.path.join(golden_dir, "dec_game_provenance.json")))
    assert set(table) == {"dec_game_configs.json", "dec_game_step.npz"}
    for f, files in table.items():
        assert os.path.isfile(os.path.join(golden_dir, f)) and os.path.getsize(os.path.join(golden_dir, f)) < 1 << 20
        assert files and all(len(h) == 64 for h in files.values()), f
        assert any(k.endswith("a1_game/dec_high_level_game_config.py") for k in files), f
    step = table["dec_game_step.npz"]
    assert any(k.endswith("a1_game/low_level_game.py") for k in step) and any(k.endswith("a1_game/dec_high_level_game.py") for k in step)
    # the other tables are untouched by this generator
    assert not any("dec_game" in k for k in json.load(open(os.path.join(golden_dir, "provenance.json"))))
    assert not any("dec_game" in k for k in json.load(open(os.path.join(golden_dir, "game_provenance.json"))))


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is only present in the build container")
def test_reference_files_still_hash_to_what_was_executed(golden_dir):
    table = json.load(open(os.path.join(golden_dir, "dec_game_provenance.json")))
    seen = {}
    for files in table.values():
        seen.update(files)
    for rel, want in sorted(seen.items()):
        got = hashlib.sha256(open(os.path.join(REF, rel)).read().encode()).hexdigest()
        assert got == want, f"{rel} changed since the fixtures were generated: regenerate with tools/make_dec_game_golden.py and review the diff"


def test_import_registers_nothing_and_register_dec_adds_the_task():
    import legged_games_gym_amd.envs.a1_game as a1_game
    from legged_games_gym_amd.envs import task_registry
    assert a1_game.TASKS == ("high_level_game",) and a1_game.DEC_TASKS == ("dec_high_level_game",)
    assert set(task_registry.task_classes) == LOCOMOTION_TASKS


def test_register_dec_and_restore(dec_registered):
    from legged_games_gym_amd.envs.a1_game import DecHighLevelGame, DecHighLevelGameCfg, DecHighLevelGameCfgPPO
    reg = dec_registered
    assert set(reg.task_classes) == LOCOMOTION_TASKS | {"dec_high_level_game"}
    assert reg.get_task_class("dec_high_level_game") is DecHighLevelGame
    env_cfg, train_cfg = reg.get_cfgs("dec_high_level_game")
    assert isinstance(env_cfg, DecHighLevelGameCfg) and isinstance(train_cfg, DecHighLevelGameCfgPPO)
    assert env_cfg.seed == train_cfg.seed == 1 and train_cfg.runner.experiment_name == "dec_high_level_game"
    assert not hasattr(DecHighLevelGame, "_sim") and hasattr(reg, "make_dec_alg_runner")


def test_registry_is_back_to_five_after_the_fixture():
    from legged_games_gym_amd.envs import task_registry
    assert set(task_registry.task_classes) == LOCOMOTION_TASKS


def test_train_script_points_to_train_dec_game():
    from legged_games_gym_amd.scripts.train import train
    from legged_games_gym_amd.utils import get_args
    with pytest.raises(SystemExit, match="train_dec_game"):
        train(get_args(["--task", "dec_high_level_game", "--headless"]))
    assert get_args(["--max_evolutions", "3"]).max_evolutions == 3 and get_args([]).max_evolutions is None


def test_evolutions_alternate_predator_first():
    from legged_games_gym_amd.rl import DecGamePolicyRunner
    assert [DecGamePolicyRunner.agent_of(e) for e in range(4)] == ["pred", "prey", "pred", "prey"]
    from legged_games_gym_amd.envs.a1_game.dec_high_level_game import SEED_OFFSET_PRED, SEED_OFFSET_PREY
    assert (SEED_OFFSET_PREY, SEED_OFFSET_PRED) == (7919, 7919 + 104729)
