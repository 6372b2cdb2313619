"""The recurrent actor launch of the game tasks without a GPU: the header's functions are ``capi.GAME_RECURRENT_SYMBOLS``
(include/legged_game_recurrent.h), a library of their own exports them and refuses bad arguments before any launch, the struct sizes it
sees, its kernel resource table, and what the runner says where ``device_rollout`` with a recurrent policy cannot run."""
import ctypes
import os
import re
import types

import pytest

from legged_games_gym_amd import capi

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
CSRC = os.path.join(REPO, "legged_games_gym_amd", "csrc")
RESOURCES = os.path.join(CSRC, "kernel_resources_game_recurrent.txt")
HEADER = "legged_game_recurrent.h"
KERNEL = "k_game_lstm_act"


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", header)).read(), flags=re.S)
    return re.findall(r"\b(lg_[a-z_0-9]+)\s*\(", text)


@pytest.fixture(scope="module")
def libs():
    if not (os.path.isfile(capi.game_recurrent_library_path()) and os.path.isfile(capi.library_path())):
        import __graft_entry__ as entry
        entry.build()
    return capi.bind_game_recurrent(ctypes.CDLL(capi.game_recurrent_library_path())), ctypes.CDLL(capi.library_path())


class _LstmActor(ctypes.Structure):
    """``struct lg_lstm_actor`` (csrc/lg_recurrent.h) in host memory: the entry point reads the shape from the handle and refuses every call
    below before it would touch the device pointers (null here)."""
    _fields_ = [("dims", ctypes.c_int32 * 5), ("pad", ctypes.c_int32 * 5), ("device", ctypes.c_int32), ("max_width", ctypes.c_int32),
                ("w_off", ctypes.c_size_t * 4), ("b_off", ctypes.c_size_t * 4), ("d_p", ctypes.c_void_p), ("d_std", ctypes.c_void_p)]


class _Policy(ctypes.Structure):
    """``struct lg_policy`` (csrc/lg_host.h) in host memory."""
    _fields_ = [("dims", ctypes.c_int32 * 5), ("tiles", ctypes.c_int * 4), ("d_w", ctypes.c_void_p * 4), ("d_b", ctypes.c_void_p * 4),
                ("d_std", ctypes.c_void_p), ("device", ctypes.c_int), ("wide", ctypes.c_bool), ("wide_ks", ctypes.c_int * 4),
                ("wide_ot", ctypes.c_int * 4), ("d_wb", ctypes.c_void_p * 4), ("d_bb", ctypes.c_void_p * 4)]


def test_header_symbol_list_matches_binding_and_is_disjoint_from_the_main_library():
    assert sorted(_declared(HEADER)) == sorted(capi.GAME_RECURRENT_SYMBOLS)
    assert {"lg_game_lstm_act", "lg_game_recurrent_last_error", "lg_game_recurrent_sizeof"} == set(capi.GAME_RECURRENT_SYMBOLS)
    assert not set(capi.GAME_RECURRENT_SYMBOLS) & set(capi.ALL_SYMBOLS)
    assert not set(capi.GAME_RECURRENT_SYMBOLS) & set(capi.LSTM_SEQ_SYMBOLS)
    assert HEADER not in capi.ABI
    for header in capi.ABI:
        assert not set(capi.GAME_RECURRENT_SYMBOLS) & set(_declared(header)), header


def test_the_new_library_exports_the_symbols_and_the_main_library_does_not(libs, monkeypatch):
    rec, main = libs
    for sym in capi.GAME_RECURRENT_SYMBOLS:
        assert hasattr(rec, sym), sym
        assert not hasattr(main, sym), sym
    assert len(rec.lg_game_lstm_act.argtypes) == 18
    import __graft_entry__ as entry
    assert entry.GAME_REC_SOURCE == "lg_game_lstm_act.hip" and entry.GAME_REC_SOURCE not in entry.HIP_SOURCES
    assert entry.HIP_SOURCES == ["lg_kernels.hip", "lg_learner.hip", "lg_game_entry.hip", "lg_game_act.hip", "lg_dec_game.hip", "lg_pursuer_game.hip",
                                 "lg_game_outcome.hip", "lg_dec_game_outcome.hip", "lg_pool_act.hip", "lg_member_outcome.hip", "lg_recurrent.hip"]
    # the main library's staleness check reads the shared actor body (lg_recurrent.hip includes it), not the new unit's public header
    assert not any("game_recurrent" in h or "game_lstm" in h for h in entry.HIP_HEADERS)
    assert "lg_lstm_actor_body.h" in entry.HIP_HEADERS
    source = open(os.path.join(CSRC, "lg_recurrent.hip")).read()
    assert '#include "lg_lstm_actor_body.h"' in source
    # ... and the new library's reads every shared header its source includes
    want = {"lg_policy.h", "lg_device.h", "lg_game_common.h", "lg_recurrent.h", "lg_host.h", "lg_lstm_actor_body.h", "lg_lib_error.h", "lg_memory_host.h"}
    assert want <= set(entry.GAME_REC_HEADERS)
    assert {os.path.basename(h) for h in entry.GAME_REC_HEADERS if os.path.isabs(h)} >= {"legged_game.h", "legged_game_recurrent.h"}
    included = set(re.findall(r'#include\s+"([^"]+)"', open(os.path.join(CSRC, entry.GAME_REC_SOURCE)).read()))
    assert {os.path.basename(i) for i in included} <= want | {"legged_game_recurrent.h"}, included
    # (self-contained at link time: the fixture's dlopen binds every function at once and would fail on a symbol only the main library has)
    monkeypatch.setenv("LG_GAME_RECURRENT_LIB", "/nonexistent/liblegged_game_recurrent.so")
    assert capi.game_recurrent_library_path() == "/nonexistent/liblegged_game_recurrent.so"


def test_struct_sizes_agree_with_the_binding(libs):
    rec, main = libs
    assert rec.lg_game_recurrent_sizeof(0) == ctypes.sizeof(capi.lg_game_params)
    assert rec.lg_game_recurrent_sizeof(1) == ctypes.sizeof(capi.lg_game_buffers)
    main.lg_game_sizeof.restype = ctypes.c_int                    # ... and with what the main library sees
    assert rec.lg_game_recurrent_sizeof(0) == main.lg_game_sizeof(0) and rec.lg_game_recurrent_sizeof(1) == main.lg_game_sizeof(1)
    assert rec.lg_game_recurrent_sizeof(2) == ctypes.sizeof(_Policy) and rec.lg_game_recurrent_sizeof(3) == ctypes.sizeof(_LstmActor)
    assert rec.lg_game_recurrent_sizeof(4) == -1 and rec.lg_game_recurrent_sizeof(-1) == -1


def test_bad_arguments_are_refused_before_any_launch(libs):
    rec, _ = libs
    hl = _LstmActor()
    hl.dims[:], hl.pad[:], hl.max_width = [256, 512, 256, 128, 6], [256, 512, 256, 128, 32], 512
    ll = _Policy()
    ll.dims[:], ll.tiles[:], ll.wide = [235, 512, 256, 128, 12], [15, 32, 16, 8], True
    P = capi.lg_game_params()
    P.num_envs = 64
    MB = 1 << 20                                                   # never dereferenced
    B = capi.game_buffers({"command": 1 * MB, "ll_commands": 2 * MB})

    def call(hl=ctypes.addressof(hl), ll=ctypes.addressof(ll), P=P, B=B, h=3 * MB, hl_obs=4 * MB, ll_obs=5 * MB, ll_actions=6 * MB, mean=7 * MB,
             obs_copy=None):
        return rec.lg_game_lstm_act(hl, ll, ctypes.byref(P) if P is not None else None, ctypes.byref(B) if B is not None else None, h, hl_obs, ll_obs,
                                    ll_actions, mean, 1, 1, None, 0, None, None, None, obs_copy, None)

    for name in ("hl", "ll", "P", "B", "h", "ll_obs", "ll_actions", "mean"):
        assert call(**{name: None}) == -1 and b"null" in rec.lg_game_recurrent_last_error(), name
    for missing in ("command", "ll_commands"):
        Bm = capi.game_buffers({k: v for k, v in (("command", 1 * MB), ("ll_commands", 2 * MB)) if k != missing})
        assert call(B=Bm) == -1 and b"null" in rec.lg_game_recurrent_last_error(), missing
    assert call(hl_obs=None, obs_copy=8 * MB) == -1 and b"null" in rec.lg_game_recurrent_last_error()
    for n in (0, -5):
        P.num_envs = n
        assert call() == -2 and b"num_envs" in rec.lg_game_recurrent_last_error(), n
    P.num_envs = 64
    for nA in (2, 12, 5, 7):                                        # six actions only
        hl.dims[4] = nA
        assert call() == -4, nA
    hl.dims[4] = 6
    ll.wide = False
    assert call() == -4                                             # the f32-only handle of a narrow actor
    ll.wide, ll.tiles[0] = True, 11
    assert call() == -4 and b"235" in rec.lg_game_recurrent_last_error()      # the wide 169-input actor
    ll.tiles[0] = 15
    # every call above returned before the launch: with these fake handles the next step would be a launch on null operands, so a valid
    # call is not made here (tests/test_gpu_game_recurrent.py makes it)


def test_kernel_resource_table_lists_exactly_the_one_kernel_without_spills():
    rows = [l for l in open(RESOURCES) if not l.startswith("#")]
    assert len(rows) == 1, rows
    assert re.match(rf"_ZN2lg{len(KERNEL)}{KERNEL}E", rows[0].split()[0]), rows[0]
    f = dict(zip(rows[0].split()[1::2], rows[0].split()[2::2]))
    assert f["spill"] == "0" and f["scratch"] == "0", rows[0]
    assert int(f["VGPRs"]) + int(f["AGPRs"]) <= 256, rows[0]      # 512 threads: two waves per SIMD
    main = open(os.path.join(CSRC, "kernel_resources.txt")).read()
    assert KERNEL not in main and "game_lstm" not in main
    assert "_ZN2lg12k_lstm_actorENS_13LstmActorArgsE" in main       # the stand-alone actor kept its symbol when its body moved to a header


def test_device_rollout_with_a_recurrent_policy_on_the_cpu_says_why_and_keeps_the_generic_loop(capsys):
    from legged_games_gym_amd.rl import OnPolicyRunner
    from legged_games_gym_amd.rl.actor_critic import ActorCriticRecurrent
    ac = ActorCriticRecurrent(19, 19, 6, [32, 32, 32], [32, 32, 32], rnn_hidden_size=32)
    game_like = types.SimpleNamespace(ll_env=object(), step_policy=lambda *a, **k: None, num_privileged_obs=None, num_envs=4)

    def make(cfg, device, env=game_like, policy=ac):
        r = OnPolicyRunner.__new__(OnPolicyRunner)
        r.cfg, r.device, r.env, r.alg, r.num_steps_per_env = cfg, device, env, types.SimpleNamespace(actor_critic=policy), 4
        capsys.readouterr()
        fused = r._make_fused_actor()
        return r, fused, capsys.readouterr().out

    r, fused, out = make({"device_rollout": True}, "cpu")
    assert fused is None and r._game_rollout is False and r._recurrent_rollout is False
    assert out.count("\n") == 1 and "device rollout unavailable" in out and "cpu" in out and "generic VecEnv loop" in out, out
    r, fused, out = make({}, "cpu")                                  # the switch is off: not a word
    assert fused is None and out == "" and r._game_rollout is False and r._recurrent_rollout is False
    # a memory the device cell does not cover names the cell's reason, a task without step_policy its own
    wide = ActorCriticRecurrent(19, 19, 6, [32, 32, 32], [32, 32, 32], rnn_hidden_size=512)
    r, fused, out = make({"device_rollout": True}, "cuda:0", policy=wide)
    assert fused is None and "512" in out and "device LSTM cell" in out and r._game_rollout is False, out
    dec_like = types.SimpleNamespace(ll_env=object(), num_privileged_obs=None, num_envs=4)
    r, fused, out = make({"device_rollout": True}, "cuda:0", env=dec_like)
    assert fused is None and "no recurrent policy for this task" in out, out


def test_the_recurrent_actor_classes_have_what_the_env_reads_of_a_fused_actor():
    from legged_games_gym_amd.rl.fused_actor import FusedActor
    from legged_games_gym_amd.rl.recurrent_actor import DeviceLstmActor, RecurrentFusedActor
    for cls in (DeviceLstmActor, RecurrentFusedActor):
        for name in ("output_buffers", "peek_step", "next_step"):
            assert callable(getattr(cls, name)), (cls.__name__, name)
    assert RecurrentFusedActor.recurrent is True and not hasattr(FusedActor, "recurrent")
    assert isinstance(RecurrentFusedActor.handle, property)
    # host and device step counting as FusedActor's, without a handle
    a = DeviceLstmActor.__new__(DeviceLstmActor)
    a.step_counter, a._host_step, a.handle = None, 0, None
    assert a.peek_step() == (1, None) and a.peek_step() == (1, None) and a.next_step() == (1, None) and a.peek_step() == (2, None)
    ctr = types.SimpleNamespace(data_ptr=lambda: 4096)
    a.step_counter = ctr
    assert a.peek_step() == (-1, 4096) and a.next_step() == (-1, 4096) and a._host_step == 1
