"""The game task's config classes equal the reference's own, value for value (tests/golden/game_configs.json = ``class_to_dict`` of the
reference's ``HighLevelGameFlatCfg / HighLevelGameFlatCfgPPO``, executed from the reference file by tools/make_game_golden.py), and the game
fixtures carry their own provenance table."""
import hashlib
import json
import os

import pytest

from legged_games_gym_amd.envs.a1_game.high_level_game_flat_config import HighLevelGameFlatCfg, HighLevelGameFlatCfgPPO
from legged_games_gym_amd.utils.helpers import class_to_dict

from tests.test_golden_provenance import REF            # where the reference tree lies when it is present (build container only)
NEW_FIELDS = {("env", "ll_policy_path"): None}        # fields this build adds to the reference's config, with their defaults


def _norm(x):
    return json.loads(json.dumps(x))


def test_game_config_values_match_reference(golden_dir):
    gold = json.load(open(os.path.join(golden_dir, "game_configs.json")))["high_level_game"]
    env, train = _norm(class_to_dict(HighLevelGameFlatCfg())), _norm(class_to_dict(HighLevelGameFlatCfgPPO()))
    for (section, key), default in NEW_FIELDS.items():
        assert key not in gold["env"][section]
        assert env[section].pop(key) == default
    assert env == gold["env"]                       # key for key
    assert train == gold["train"]
    assert list(env["rewards"]["scales"]) == ["evasion", "pursuit"]          # dir() order = the reward summation order


def test_game_configs_are_instances_not_shared_classes():
    a, b = HighLevelGameFlatCfg(), HighLevelGameFlatCfg()
    a.env.num_envs = 7
    assert b.env.num_envs == 2000 and HighLevelGameFlatCfg.env.num_envs == 2000


def test_game_provenance_lists_the_fixtures(golden_dir):
    table = json.load(open(os.path.join(golden_dir, "game_provenance.json")))
    assert set(table) == {"game_configs.json", "game_step.npz", "game_reset.npz"}
    for f, files in table.items():
        assert os.path.isfile(os.path.join(golden_dir, f))
        assert files and all(len(h) == 64 for h in files.values()), f
        assert any(k.endswith("a1_game/high_level_game_flat_config.py") for k in files), f
    for f in ("game_step.npz", "game_reset.npz"):
        assert any(k.endswith("a1_game/low_level_game.py") for k in table[f]) and any(k.endswith("a1_game/high_level_game.py") for k in table[f])
    # the locomotion table is untouched by the game generator
    assert not any(k.startswith("game_") for k in json.load(open(os.path.join(golden_dir, "provenance.json"))))


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is only present in the build container")
def test_game_reference_files_still_hash_to_what_was_executed(golden_dir):
    table = json.load(open(os.path.join(golden_dir, "game_provenance.json")))
    seen = {}
    for files in table.values():
        seen.update(files)
    for rel, want in sorted(seen.items()):
        got = hashlib.sha256(open(os.path.join(REF, rel)).read().encode()).hexdigest()
        assert got == want, f"{rel} changed since the fixtures were generated: regenerate with tools/make_game_golden.py and review the diff"
