"""The privileged (critic-only) observations of ``dec_high_level_game`` without a GPU: the width check of the two config fields, the NumPy
twin's own sanity (tests/dec_privileged_twin.py), the header's constants and functions against ``capi``
(include/legged_dec_game_privileged.h), the library of its own that exports them and refuses bad arguments before any launch, and a GPU
reference test for every kernel it compiled (csrc/kernel_resources_dec_game_privileged.txt), in the manner of
tests/test_dec_game_recurrent_abi.py and tests/test_dec_game_recurrent_kernel_coverage.py."""
import ast
import ctypes
import os
import re

import numpy as np
import pytest

from legged_games_gym_amd import capi
from tests import dec_privileged_twin as pt
from tests.dec_game_fixtures import synthetic_state
from tests.test_actor_kernel_coverage import kernel_of

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
CSRC = os.path.join(REPO, "legged_games_gym_amd", "csrc")
RESOURCES = os.path.join(CSRC, "kernel_resources_dec_game_privileged.txt")
HEADER = "legged_dec_game_privileged.h"
KERNELS = ("k_privileged_obs",)
GPU = "tests/test_gpu_dec_privileged.py"
MB = 1 << 20                                                       # "device addresses" that are never dereferenced
F = np.float32

COVERAGE = {
    # designed states at 1 / 33 / 65 / 257 envs against the float64 twin, guard rows, one destination alone; the rows of a reset env
    "_ZN2lg16k_privileged_obsENS_14PrivilegedArgsE": [f"{GPU}::test_kernel_matches_the_twin_on_designed_states",
                                                      f"{GPU}::test_reset_rows_are_the_twin_of_the_post_reset_state"],
}


# ----------------------------------------------------------------------------- the width check
def test_width_check_takes_none_or_the_compiled_widths_and_names_both_numbers():
    from legged_games_gym_amd.envs.a1_game.dec_high_level_game import check_privileged_widths
    assert check_privileged_widths(None, None) == ()
    assert check_privileged_widths(22, 10) == ("pred", "prey")
    assert check_privileged_widths(22, None) == ("prey",) and check_privileged_widths(None, 10) == ("pred",)
    for prey, pred in ((16, None), (None, 3), (10, 22), (22, 22), (10, 10), (23, 10), (22, 9), (0, None), (None, 0), (True, None), ("22", None), (22.5, 10)):
        with pytest.raises(ValueError, match=r"22.*10"):
            check_privileged_widths(prey, pred)
    assert (capi.LG_DEC_NUM_PRIV_PREY, capi.LG_DEC_NUM_PRIV_PRED) == (22, 10) == (pt.NUM_PRIV_PREY, pt.NUM_PRIV_PRED)


def test_single_policy_games_say_why_they_have_no_privileged_critic():
    src = open(os.path.join(REPO, "legged_games_gym_amd", "envs", "a1_game", "high_level_game.py")).read()
    assert "obs[16:19]" in src and "NotImplementedError" in src and "num_privileged_obs_prey" in src


# ----------------------------------------------------------------------------- the twin
def test_twin_relative_position_is_the_visible_observation_bit_for_bit():
    p = pt.params()
    s = synthetic_state(p, 257, seed=11, step=5)
    out, info = pt.post(dict(p, num_envs=257), s, step=5)
    prey, pred = pt.privileged32(p, out)
    vis = out["obs_prey"][:, 15] == 1
    assert vis.sum() >= 64 and (~vis).sum() >= 32 and np.array_equal(vis, info["visible"])
    np.testing.assert_array_equal(prey[vis, 16:19].view(np.uint32), np.ascontiguousarray(out["obs_prey"][vis, 9:12]).view(np.uint32))
    assert (prey[~vis, 16:19] != out["obs_prey"][~vis, 9:12]).any(axis=1).all()        # what the sensor hides
    np.testing.assert_array_equal(prey[:, :16], out["obs_prey"])
    np.testing.assert_array_equal(pred[:, :3], out["obs_pred"])
    np.testing.assert_array_equal(pred[:, 5:8], out["root_states"][:, 7:10])
    np.testing.assert_array_equal(pred[:, 8], out["obs_prey"][:, 15])
    np.testing.assert_array_equal(prey[:, 19:21], pred[:, 3:5])
    assert np.allclose(np.hypot(prey[:, 19], prey[:, 20]), 1.0, atol=1e-6)             # a unit vector for a yaw-only quaternion
    done = info["done"]
    assert done.any() and (prey[done, 21] == 1).all()                                   # a reset row: the clock starts over ...
    assert (prey[done, :9] == F(p["max_rel_pos"])).all() and (prey[done, 12:15] == 0).all()      # ... behind the cleared history


def test_twin_clock_is_exactly_one_at_zero_and_zero_at_the_limit():
    for L in (1, 2, 3, 7, 1000, 1001, 4099):
        p = pt.params(max_episode_length=L)
        ep = np.array([0, L, 1, L - 1], np.int64)
        c32, c64 = pt.clock32(p, ep), pt.clock64(p, ep)
        assert c32.dtype == F and c32[0] == 1 and c32[1] == 0 and c64[0] == 1 and c64[1] == 0
        np.testing.assert_array_equal(c32, c64.astype(F))                              # no double rounding: n / d of small integers
        assert (c32[2:] >= 0).all() and (c32[2:] <= 1).all()
    assert pt.clock32(pt.params(), np.array([1500]))[0] == F(-0.5)                      # no clamp


def test_twin_forward_vector_against_the_yaw():
    yaw = np.array([0.0, 0.4, 2.0, -2.6, -0.9, np.pi])
    quat = np.stack((0 * yaw, 0 * yaw, np.sin(yaw / 2), np.cos(yaw / 2)), axis=1).astype(F)
    fx, fy = pt.forward64(quat)
    assert np.allclose(fx, np.cos(yaw), atol=1e-6) and np.allclose(fy, np.sin(yaw), atol=1e-6)
    fx, fy = pt.forward64(np.zeros((1, 4), F))                                          # a zero quaternion: the guard of the normalisation
    assert fx[0] == 1.0 and fy[0] == 0.0


def test_designed_states_cover_both_sides_of_the_field_of_view():
    p = pt.params()
    for n in (33, 65, 257):
        s, vis = pt.designed_state(p, n)
        assert vis.sum() * 4 >= n and (~vis).sum() * 4 >= n, (n, int(vis.sum()))
        assert set(s["episode_length_buf"].tolist()) == {0, 1, 999, 1000}
        fx, fy = pt.forward64(s["root_states"][:, 3:7])
        assert {(bool(a > 0), bool(b > 0)) for a, b in zip(fx, fy)} == {(True, True), (True, False), (False, True), (False, False)}
    singles = [pt.designed_state(p, 1, first=k)[1][0] for k in range(8)]
    assert sum(singles) >= 2 and sum(not v for v in singles) >= 2


# ----------------------------------------------------------------------------- header, binding, library
def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", header)).read(), flags=re.S)
    return re.findall(r"\b(lg_[a-z_0-9]+)\s*\(", text)


@pytest.fixture(scope="module")
def libs():
    paths = (capi.dec_game_privileged_library_path(), capi.library_path(), capi.dec_game_recurrent_library_path())
    if not all(os.path.isfile(p) for p in paths):
        import __graft_entry__ as entry
        entry.build()
    return (capi.bind_dec_game_privileged(ctypes.CDLL(paths[0])),) + tuple(ctypes.CDLL(p) for p in paths[1:])


def test_header_constants_and_symbols_match_the_binding():
    text = open(os.path.join(REPO, "include", HEADER)).read()
    consts = {k: int(v) for k, v in re.findall(r"#define\s+(LG_DEC_NUM_PRIV_[A-Z]+)\s+(\d+)", text)}
    assert consts == {"LG_DEC_NUM_PRIV_PREY": capi.LG_DEC_NUM_PRIV_PREY, "LG_DEC_NUM_PRIV_PRED": capi.LG_DEC_NUM_PRIV_PRED}
    assert sorted(_declared(HEADER)) == sorted(capi.DEC_GAME_PRIVILEGED_SYMBOLS)
    assert {"lg_dec_game_privileged_obs", "lg_dec_game_privileged_sizeof", "lg_dec_game_privileged_last_error"} == set(capi.DEC_GAME_PRIVILEGED_SYMBOLS)
    for other in (capi.ALL_SYMBOLS, capi.LSTM_SEQ_SYMBOLS, capi.GAME_RECURRENT_SYMBOLS, capi.DEC_GAME_RECURRENT_SYMBOLS, capi.DEC_POOL_RECURRENT_SYMBOLS):
        assert not set(capi.DEC_GAME_PRIVILEGED_SYMBOLS) & set(other)
    assert HEADER not in capi.ABI
    for header in list(capi.ABI) + ["legged_game_recurrent.h", "legged_lstm_sequence.h", "legged_dec_game_recurrent.h", "legged_dec_pool_recurrent.h"]:
        assert not set(capi.DEC_GAME_PRIVILEGED_SYMBOLS) & set(_declared(header)), header


def test_the_library_exports_the_symbols_and_is_built_from_its_own_source(libs, monkeypatch):
    priv, *others = libs
    for sym in capi.DEC_GAME_PRIVILEGED_SYMBOLS:
        assert hasattr(priv, sym), sym
        for lib in others:
            assert not hasattr(lib, sym), (sym, lib._name)
    for sym in ("lg_dec_game_post", "lg_dec_lstm_step", "lg_step"):
        assert not hasattr(priv, sym), sym                         # ... and it holds nothing of theirs
    assert len(priv.lg_dec_game_privileged_obs.argtypes) == 5
    import __graft_entry__ as entry
    assert entry.DEC_GAME_PRIV_SOURCE == "lg_dec_game_privileged.hip" and entry.DEC_GAME_PRIV_SOURCE not in entry.HIP_SOURCES
    assert not any(os.path.basename(h) == HEADER for h in entry.HIP_HEADERS)       # the main library's staleness check does not read it
    included = {os.path.basename(i) for i in re.findall(r'#include\s+"([^"]+)"', open(os.path.join(CSRC, entry.DEC_GAME_PRIV_SOURCE)).read())}
    assert included <= {os.path.basename(h) for h in entry.DEC_GAME_PRIV_HEADERS}, included
    assert {"lg_dec_game_post.h", HEADER} <= included
    monkeypatch.setenv("LG_DEC_GAME_PRIVILEGED_LIB", "/nonexistent/liblegged_dec_game_privileged.so")
    assert capi.dec_game_privileged_library_path() == "/nonexistent/liblegged_dec_game_privileged.so"
    monkeypatch.setattr(capi.LIBRARIES["dec_game_privileged"], "handle", None)
    with pytest.raises(RuntimeError, match=r"is not built; run .*build\(\)"):
        capi.load_dec_game_privileged_library()


def test_struct_sizes_agree_with_the_binding_and_the_main_library(libs):
    priv, main = libs[0], libs[1]
    main.lg_dec_game_sizeof.restype = ctypes.c_int
    for which, st in ((0, capi.lg_dec_game_params), (1, capi.lg_dec_game_buffers)):
        assert priv.lg_dec_game_privileged_sizeof(which) == ctypes.sizeof(st) == main.lg_dec_game_sizeof(which), which
    assert priv.lg_dec_game_privileged_sizeof(2) == -1 and priv.lg_dec_game_privileged_sizeof(-1) == -1
    assert capi.DEC_GAME_PRIVILEGED_STRUCTS == {0: capi.lg_dec_game_params, 1: capi.lg_dec_game_buffers}


def test_launch_refuses_bad_arguments_before_any_launch(libs):
    priv = libs[0]
    err = priv.lg_dec_game_privileged_last_error
    P = capi.lg_dec_game_params()
    P.num_envs, P.max_episode_length = 64, 1000
    full = {"predator_pos": 1 * MB, "ll_root_states": 2 * MB, "obs_prey": 3 * MB, "obs_pred": 4 * MB, "episode_length_buf": 5 * MB}
    B = capi.dec_game_buffers(full)

    def call(P=P, B=B, pred=6 * MB, prey=7 * MB):
        return priv.lg_dec_game_privileged_obs(ctypes.byref(P) if P is not None else None, ctypes.byref(B) if B is not None else None, pred, prey, None)

    assert call(P=None) == -1 and b"null" in err()
    assert call(B=None) == -1 and b"null" in err()
    assert call(pred=None, prey=None) == -1 and b"both destinations" in err()          # nothing launched
    for missing in full:
        rc = call(B=capi.dec_game_buffers({k: v for k, v in full.items() if k != missing}))
        assert rc == -1 and b"null" in err(), missing
    # the predator's observations are read for the predator's rows only (refused above with both destinations; with the prey's alone the
    # next step would be a launch on these fake addresses, so that call is not made here)
    for n in (0, -4):
        P.num_envs = n
        assert call() == -2 and b"num_envs" in err(), n
    P.num_envs = 64
    for L in (0, -1):
        P.max_episode_length = L
        assert call() == -2 and b"max_episode_length" in err(), L
    # every call above returned before the launch (tests/test_gpu_dec_privileged.py makes the valid ones)


# ----------------------------------------------------------------------------- kernel resources and coverage
def compiled(path=RESOURCES):
    with open(path) as f:
        return {line.split()[0] for line in f if line.strip() and not line.startswith("#")}


def uncovered(path=RESOURCES):
    return sorted(compiled(path) - set(COVERAGE))


def test_kernel_resource_table_lists_the_one_kernel_without_spills():
    rows = [l for l in open(RESOURCES) if not l.startswith("#")]
    assert len(rows) == 1, rows
    assert {kernel_of(r.split()[0]) for r in rows} == set(KERNELS)
    f = dict(zip(rows[0].split()[1::2], rows[0].split()[2::2]))
    assert f["spill"] == "0" and f["scratch"] == "0" and f["LDS"] == "0" and int(f["VGPRs"]) <= 64 and f["occupancy"] == "8", rows[0]
    from tests.test_dec_pool_abi import FORBIDDEN                  # substrings the existing ABI tests count rows by
    for sub in FORBIDDEN:
        assert sub not in rows[0], sub
    for name in os.listdir(CSRC):                                  # ... and no other table lists it
        if name.startswith("kernel_resources") and name != os.path.basename(RESOURCES):
            assert KERNELS[0] not in open(os.path.join(CSRC, name)).read(), name


def test_every_kernel_of_the_library_has_a_reference_test():
    names = compiled()
    assert {kernel_of(n) for n in names} == set(KERNELS), sorted(names)
    assert len(names) == len(COVERAGE) == 1
    assert uncovered() == [], "kernels no GPU test compares with a reference: " + ", ".join(uncovered())
    assert set(COVERAGE) == names, "table entries for kernels that are no longer compiled: " + ", ".join(sorted(set(COVERAGE) - names))


def test_every_named_test_function_exists_in_a_gpu_module():
    with open(os.path.join(REPO, GPU)) as f:
        tree = ast.parse(f.read())
    assert any(isinstance(n, ast.Assign) and any(getattr(x, "id", None) == "pytestmark" for x in n.targets) and "gpu" in ast.unparse(n.value)
               for n in tree.body), f"{GPU} is not marked gpu"
    funcs = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    for tests in COVERAGE.values():
        assert tests
        for t in tests:
            path, func = t.split("::")
            assert path == GPU and func in funcs, t


def test_a_further_instantiation_is_reported_uncovered(tmp_path):
    extra = ["_ZN2lg16k_privileged_obsILb1EEEvNS_14PrivilegedArgsE"]
    assert not set(extra) & set(COVERAGE)
    copy = tmp_path / "kernel_resources_dec_game_privileged.txt"
    with open(RESOURCES) as f:
        text = f.read()
    copy.write_text(text + "".join(f"{e}  VGPRs 64  AGPRs 0  spill 0  scratch 0  LDS 0  occupancy 8\n" for e in extra))
    assert uncovered(str(copy)) == sorted(extra)
    assert uncovered() == []
