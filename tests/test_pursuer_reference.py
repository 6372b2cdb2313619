"""The scripted pursuer without a GPU: tests/pursuer_twin.py (the NumPy float32 restatement of csrc/lg_pursuer_game.hip) reproduces the
reference's own ``HighLevelGame.step`` driven by its own ``full_obs_predator`` as recorded in tests/golden/pursuer_step.npz
(tools/make_pursuer_golden.py); the clamp's corner cases; the config, the registry, the C-ABI, the resource table and the provenance.

Bounds as tests/test_game_reference.py: the velocity, the integrated position and everything that is copied, added, subtracted or
multiplied are BIT-equal on every env; the reward may differ by 4 ulp of its largest intermediate."""
import ctypes
import hashlib
import json
import os
import re

import numpy as np
import pytest

from legged_games_gym_amd import capi
from legged_games_gym_amd.utils.helpers import class_to_dict
from tests import game_twin as tw
from tests import pursuer_twin as pt
from tests.game_fixtures import LOCOMOTION_TASKS, check_call, load
from tests.pursuer_fixtures import pursuer_calls
from tests.test_golden_provenance import REF            # where the reference tree lies when it is present (build container only)

F = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
RESOURCES = os.path.join(REPO, "legged_games_gym_amd", "csrc", "kernel_resources.txt")


# ----------------------------------------------------------------------------- fixture
@pytest.mark.parametrize("tag,calls", [("a", 4), ("b", 3)])
def test_twin_reproduces_the_reference_step_with_its_scripted_predator(golden_dir, tag, calls):
    g = load(golden_dir, "pursuer_step.npz")
    assert "command=None" in str(g["departure"]) and "188" in str(g["departure"])          # the one departure is stated in the fixture
    assert os.path.getsize(os.path.join(golden_dir, "pursuer_step.npz")) <= os.path.getsize(os.path.join(golden_dir, "game_step.npz"))
    q = json.loads(str(g[f"{tag}_pursuer_params"]))
    assert q == pt.pursuer_params() and g[f"{tag}_env_origins"].shape[0] == 512
    assert (json.loads(str(g[f"{tag}_params"]))["env_radius"] >= 0) == (tag == "b")
    n = 0
    for k, p, q, s, out, info, want in pursuer_calls(g, tag):
        tw.assert_margins(p, info)
        np.testing.assert_array_equal(info["ep"], want["ep"])                                 # the post-increment step count
        np.testing.assert_array_equal(info["ep"], s["curr_episode_step"] + 1)
        np.testing.assert_array_equal(info["predator_command"].view(np.uint32), want["predator_command"].view(np.uint32))
        np.testing.assert_array_equal(info["predator_integrated"].view(np.uint32), want["predator_integrated"].view(np.uint32))
        np.testing.assert_array_equal(s["command"].view(np.uint32), want["command"].view(np.uint32))          # columns 4:6 are clipped, stored, ignored
        np.testing.assert_array_equal(info["visible"], want["sense_flag"] != 0)
        np.testing.assert_array_equal(out["obs"][:, 9:12].view(np.uint32), want["sense_pos"].view(np.uint32))
        check_call(p, s, out, info, want)
        # the three branches of the rule, in every call of the committed fixture
        unsat, sat, neg = pt.branch_shares(info)
        assert min(unsat, sat, neg) >= 0.05, (tag, k, unsat, sat, neg)
        assert (info["ep"][info["lim"] < 0] > q["max_episode_length"]).all() and (info["lim"][info["ep"] <= q["max_episode_length"]] > 0).all()
        assert (info["predator_command"][info["lim"] < 0] == info["lim"][info["lim"] < 0, None]).all()       # min > max: the clamp returns max
        # the move differs from what columns 4:6 of the command would have given
        assert not np.array_equal(tw.integrate_predator(p, s["predator_pos"], s["command"]), info["predator_integrated"])
        assert not info["visible"][0] and not out["reset_buf"][0]                             # env 0: occluded and alive
        assert out["reset_buf"].any() and info["capture"].any()
        n += 1
    assert n == calls


# ----------------------------------------------------------------------------- the clamp
def test_speed_limit_and_clamp_corner_cases():
    q = pt.pursuer_params()
    L = q["max_episode_length"]
    assert pt.speed_limit(q, np.array([0]))[0] == F(q["max_lin_vel"])
    assert pt.speed_limit(q, np.array([L]))[0] == F(q["min_lin_vel"])
    ep = np.arange(0, 2 * L + 1)
    lim = pt.speed_limit(q, ep)
    assert (np.diff(lim) < 0).all() and lim[-1] < 0                                           # the pursuer "loses steam", then backs away
    # lim < 0: torch.clamp with min > max returns max -- v == lim on both axes whatever the prey's position
    late = np.array([L + 10, L + 500, 2 * L])
    for d in (50.0, -50.0, 0.0, 1e-4):
        v, lim = pt.velocity(q, np.full((3, 2), d, F), np.zeros((3, 2), F), late)
        assert (lim < 0).all() and (v == lim[:, None]).all()
    # lim > 0: saturated at +-lim far away, gain x relative position close by
    v, lim = pt.velocity(q, np.array([[50.0, -50.0], [0.25, -0.125]], F), np.zeros((2, 2), F), np.array([500, 500]))
    assert v[0].tolist() == [lim[0], -lim[0]] and v[1].tolist() == [0.5, -0.25]
    # another gain and limits: the parameters are read, not the literals
    q2 = pt.pursuer_params(max_lin_vel=1.0, min_lin_vel=0.5, gain=4.0, max_episode_length=10)
    v, lim = pt.velocity(q2, np.array([[0.125, 9.0]], F), np.zeros((1, 2), F), np.array([5]))
    assert lim[0] == F(0.75) and v[0].tolist() == [0.5, 0.75]


# ----------------------------------------------------------------------------- config, registry
def test_config_is_the_parents_plus_one_section():
    from legged_games_gym_amd.envs.a1_game import HighLevelGameFlatCfg, HighLevelGameFlatCfgPPO, ScriptedPredatorGameCfg, ScriptedPredatorGameCfgPPO
    env = class_to_dict(ScriptedPredatorGameCfg())
    assert env.pop("predator") == {"max_lin_vel": 2.0, "min_lin_vel": 0.01, "gain": 2.0}
    assert env == class_to_dict(HighLevelGameFlatCfg())
    assert "predator" not in class_to_dict(HighLevelGameFlatCfg())
    train, parent = class_to_dict(ScriptedPredatorGameCfgPPO()), class_to_dict(HighLevelGameFlatCfgPPO())
    assert train["runner"].pop("experiment_name") == "scripted_predator_game" and parent["runner"].pop("experiment_name") == "high_level_game_flat"
    assert train == parent


@pytest.mark.parametrize("field,value,match", [("max_lin_vel", 0.001, "max_lin_vel"), ("gain", 0.0, "gain"), ("gain", -1.0, "gain")])
def test_construction_refuses_a_bad_rule(field, value, match):
    """Before the low-level env is built: no GPU and no checkpoint are needed to be told."""
    from legged_games_gym_amd.envs.a1_game import ScriptedPredatorGame, ScriptedPredatorGameCfg
    cfg = ScriptedPredatorGameCfg()
    setattr(cfg.predator, field, value)
    with pytest.raises(ValueError, match=match):
        ScriptedPredatorGame(cfg, None, None, "cpu", True)
    assert ScriptedPredatorGameCfg().predator.gain == 2.0 and ScriptedPredatorGameCfg.predator.max_lin_vel == 2.0


def test_register_scripted_adds_one_task_and_unregister_restores():
    from legged_games_gym_amd.envs import a1_game, task_registry
    assert a1_game.SCRIPTED_TASKS == ("scripted_predator_game",) and a1_game.TASKS == ("high_level_game",) and a1_game.DEC_TASKS == ("dec_high_level_game",)
    assert set(task_registry.task_classes) == LOCOMOTION_TASKS
    try:
        a1_game.register_scripted()
        a1_game.register_scripted()                                                           # idempotent
        assert set(task_registry.task_classes) == set(task_registry.env_cfgs) == set(task_registry.train_cfgs) == LOCOMOTION_TASKS | {"scripted_predator_game"}
        assert task_registry.get_task_class("scripted_predator_game") is a1_game.ScriptedPredatorGame
        assert issubclass(a1_game.ScriptedPredatorGame, a1_game.HighLevelGame)
        env_cfg, train_cfg = task_registry.get_cfgs("scripted_predator_game")
        assert isinstance(env_cfg, a1_game.ScriptedPredatorGameCfg) and train_cfg.runner.experiment_name == "scripted_predator_game"
    finally:
        a1_game.unregister_scripted()
    assert set(task_registry.task_classes) == set(task_registry.env_cfgs) == set(task_registry.train_cfgs) == LOCOMOTION_TASKS
    try:
        a1_game.register()                                                                    # still adds only high_level_game
        assert set(task_registry.task_classes) == LOCOMOTION_TASKS | {"high_level_game"}
    finally:
        a1_game.unregister()
    assert set(task_registry.task_classes) == LOCOMOTION_TASKS


# ----------------------------------------------------------------------------- C-ABI, resource table
def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", header)).read(), flags=re.S)
    return re.findall(r"\b(lg_[a-z_0-9]+)\s*\(", text)


def test_library_exports_the_symbols_with_the_ctypes_layout():
    assert sorted(_declared("legged_pursuer_game.h")) == sorted(capi.PURSUER_SYMBOLS)
    assert not set(capi.PURSUER_SYMBOLS) & (set(capi.GAME_SYMBOLS) | set(capi.DEC_GAME_SYMBOLS) | set(capi.EXPORTED_SYMBOLS))
    path = capi.library_path()
    if not os.path.isfile(path):
        import __graft_entry__ as entry
        entry.build()
    lib = ctypes.CDLL(path)
    for sym in capi.PURSUER_SYMBOLS:
        assert hasattr(lib, sym), sym
    capi.bind_header(lib, "legged_pursuer_game.h")                                                         # raises on a layout mismatch
    assert lib.lg_pursuer_sizeof(0) == ctypes.sizeof(capi.lg_pursuer_params) and lib.lg_pursuer_sizeof(1) == -1
    assert ctypes.sizeof(capi.lg_pursuer_params) % 8 == 0
    assert [n for n, _ in capi.lg_pursuer_params._fields_] == ["max_lin_vel", "min_lin_vel", "gain", "max_episode_length"]
    # refused before anything is launched (no GPU needed): null arguments, then the ranges
    lib.lg_last_error.restype = ctypes.c_char_p
    P, Q, B = capi.lg_game_params(), capi.lg_pursuer_params(), capi.game_buffers({})
    P.num_envs, P.decimation = 4, 4
    Q.max_lin_vel, Q.min_lin_vel, Q.gain, Q.max_episode_length = 2.0, 0.01, 2.0, 1000
    for args in ((None, None, None), (None, ctypes.byref(Q), ctypes.byref(B)), (ctypes.byref(P), None, ctypes.byref(B)), (ctypes.byref(P), ctypes.byref(Q), None)):
        assert lib.lg_pursuer_post(args[0], args[1], args[2], None, 0, None) == -1
        assert b"null" in lib.lg_last_error()
    assert lib.lg_pursuer_post(ctypes.byref(P), ctypes.byref(Q), ctypes.byref(B), None, 0, None) == -1          # every buffer pointer is null
    for name, bad in (("max_episode_length", 0), ("max_episode_length", (1 << 20) + 1), ("max_lin_vel", 0.001), ("gain", 0.0)):
        R = capi.lg_pursuer_params.from_buffer_copy(Q)
        setattr(R, name, bad)
        assert lib.lg_pursuer_post(ctypes.byref(P), ctypes.byref(R), ctypes.byref(B), None, 0, None) == -2, name
        assert name.encode() in lib.lg_last_error()
    P.num_envs = 0
    assert lib.lg_pursuer_post(ctypes.byref(P), ctypes.byref(Q), ctypes.byref(B), None, 0, None) == -2


def test_resource_table_has_one_row_for_the_new_kernel():
    rows = {l.split()[0]: l.rstrip("\n") for l in open(RESOURCES) if not l.startswith("#")}
    mine = [r for n, r in rows.items() if "k_pursuer_post" in n]
    assert len(mine) == 1
    assert "spill 0" in mine[0] and "scratch 0" in mine[0] and "LDS 0" in mine[0] and "AGPRs 0" in mine[0]
    for part in ("k_game_", "k_prey_act", "k_dec_", "k_step", "k_physics"):                   # the substring counts of the existing tests
        assert part not in mine[0]
    assert sum("k_game_post" in n for n in rows) == 1 and sum(("k_step" in n or "k_physics" in n) for n in rows) == 32


# ----------------------------------------------------------------------------- provenance
def test_provenance_lists_the_fixture(golden_dir):
    table = json.load(open(os.path.join(golden_dir, "pursuer_provenance.json")))
    assert set(table) == {"pursuer_step.npz"}
    files = table["pursuer_step.npz"]
    assert os.path.getsize(os.path.join(golden_dir, "pursuer_step.npz")) < 1 << 20
    assert files and all(re.fullmatch(r"[0-9a-f]{64}", h) for h in files.values())
    assert any(k.endswith("a1_game/high_level_game.py") for k in files) and any(k.endswith("a1_game/low_level_game.py") for k in files)
    for other in ("provenance.json", "game_provenance.json", "dec_game_provenance.json"):     # the other tables are untouched by this generator
        assert not any("pursuer" in k for k in json.load(open(os.path.join(golden_dir, other))))
    if os.path.isdir(REF):                                                                    # the reference tree: build container only
        for rel, want in sorted(files.items()):
            got = hashlib.sha256(open(os.path.join(REF, rel)).read().encode()).hexdigest()
            assert got == want, f"{rel} changed since the fixture was generated: regenerate with tools/make_pursuer_golden.py and review the diff"
