"""The wide LSTM cell and actor (include/legged_recurrent_wide.h, liblegged_lstm_wide.so) without a GPU: the header's functions are
``capi.LSTM_WIDE_SYMBOLS``, a library of their own exports them and refuses bad shapes and null arguments before any launch, its kernel
resource rows, ``lstm_unsupported_reason`` with and without ``wide``, and what the runners do with the key ``wide_memory``."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch.nn as nn

from legged_games_gym_amd import capi

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
CSRC = os.path.join(REPO, "legged_games_gym_amd", "csrc")
RESOURCES = os.path.join(CSRC, "kernel_resources_lstm_wide.txt")
HEADER = "legged_recurrent_wide.h"
KERNELS = ("k_lstm_wide_cell", "k_lstm_wide_pack", "k_lstm_wide_actor", "k_lstm_wide_actor_pack")


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", header)).read(), flags=re.S)
    return re.findall(r"\b(lg_[a-z_0-9]+)\s*\(", text)


@pytest.fixture(scope="module")
def libs():
    if not (os.path.isfile(capi.lstm_wide_library_path()) and os.path.isfile(capi.library_path())):
        import __graft_entry__ as entry
        entry.build()
    return capi.bind_lstm_wide(ctypes.CDLL(capi.lstm_wide_library_path())), ctypes.CDLL(capi.library_path())


def test_header_symbol_list_matches_binding_and_is_disjoint_from_the_other_libraries():
    assert sorted(_declared(HEADER)) == sorted(capi.LSTM_WIDE_SYMBOLS)
    assert len(capi.LSTM_WIDE_SYMBOLS) == 9 and all(s.startswith("lg_lstm_wide_") for s in capi.LSTM_WIDE_SYMBOLS)
    for other in (capi.ALL_SYMBOLS, capi.LSTM_SEQ_SYMBOLS, capi.GAME_RECURRENT_SYMBOLS, capi.DEC_GAME_RECURRENT_SYMBOLS, capi.DEC_POOL_RECURRENT_SYMBOLS,
                  capi.DEC_GAME_PRIVILEGED_SYMBOLS):
        assert not set(capi.LSTM_WIDE_SYMBOLS) & set(other)
    assert HEADER not in capi.ABI
    text = open(os.path.join(REPO, "include", HEADER)).read()
    for name, value in (("LG_LSTM_WIDE_MAX_IN", capi.LG_LSTM_WIDE_MAX_IN), ("LG_LSTM_WIDE_MAX_HIDDEN", capi.LG_LSTM_WIDE_MAX_HIDDEN),
                        ("LG_LSTM_WIDE_GROUP_UNITS", capi.LG_LSTM_WIDE_GROUP_UNITS), ("LG_LSTM_WIDE_BLOCK_ENVS", capi.LG_LSTM_WIDE_BLOCK_ENVS)):
        assert re.search(rf"#define {name} {value}\b", text), name
    assert capi.LG_LSTM_WIDE_MAX_HIDDEN == 512 and capi.LG_LSTM_MAX_HIDDEN == 256
    # the signatures are those of the lg_lstm_* entries
    for wide, narrow in (("lg_lstm_wide_create", "lg_lstm_create"), ("lg_lstm_wide_load_device", "lg_lstm_load_device"), ("lg_lstm_wide_step", "lg_lstm_step"),
                         ("lg_lstm_wide_actor_create", "lg_lstm_actor_create"), ("lg_lstm_wide_actor_load_device", "lg_lstm_actor_load_device"),
                         ("lg_lstm_wide_actor_act", "lg_lstm_actor_act"), ("lg_lstm_wide_destroy", "lg_lstm_destroy"),
                         ("lg_lstm_wide_actor_destroy", "lg_lstm_actor_destroy")):
        assert capi.LSTM_WIDE_ABI[wide] == capi.ABI["legged_recurrent.h"][0][narrow], wide


def test_the_new_library_exports_the_symbols_and_the_main_library_does_not(libs, monkeypatch):
    wide, main = libs
    for sym in capi.LSTM_WIDE_SYMBOLS:
        assert hasattr(wide, sym), sym
        assert not hasattr(main, sym), sym
    import __graft_entry__ as entry
    assert entry.LSTM_WIDE_SOURCE == "lg_lstm_wide.hip" and entry.LSTM_WIDE_SOURCE not in entry.HIP_SOURCES
    assert not any("recurrent_wide" in h or "lstm_wide" in h for h in entry.HIP_HEADERS)
    included = set(re.findall(r'#include\s+"([^"]+)"', open(os.path.join(CSRC, entry.LSTM_WIDE_SOURCE)).read()))
    assert {os.path.basename(i) for i in included} == {os.path.basename(h) for h in entry.LSTM_WIDE_HEADERS}, included
    monkeypatch.setenv("LG_LSTM_WIDE_LIB", "/nonexistent/liblegged_lstm_wide.so")
    assert capi.lstm_wide_library_path() == "/nonexistent/liblegged_lstm_wide.so"
    monkeypatch.setattr(capi.LIBRARIES["lstm_wide"], "handle", None)
    with pytest.raises(RuntimeError, match="not built; run"):
        capi.load_lstm_wide_library()


def test_supported_shapes():
    ok = [(1, 32), (256, 512), (3, 288), (48, 480), (235, 512), (19, 64)]
    bad = [(0, 512), (257, 512), (48, 544), (48, 48), (48, 0), (48, 16), (-1, 64)]
    assert all(capi.lstm_wide_supported(*s) for s in ok) and not any(capi.lstm_wide_supported(*s) for s in bad)
    assert not capi.lstm_supported(48, 288) and capi.lstm_supported(48, 256)


def test_bad_shapes_and_null_arguments_are_refused_before_any_launch(libs):
    wide, _ = libs
    err = wide.lg_lstm_wide_last_error
    out = ctypes.c_void_p()
    w = np.zeros(8, np.float32).ctypes.data                        # never read: every call below returns before the upload
    for num_in, hidden in ((48, 544), (48, 48), (48, 0), (48, 1024), (0, 512), (257, 512), (-3, 64)):
        assert wide.lg_lstm_wide_create(num_in, hidden, w, w, w, w, 0, ctypes.byref(out)) == -4, (num_in, hidden)
        assert (b"hidden" in err() or b"num_in" in err()) and not out.value
    for k in range(4):
        args = [w, w, w, w]
        args[k] = None
        assert wide.lg_lstm_wide_create(48, 512, *args, 0, ctypes.byref(out)) == -1 and b"null" in err()
    assert wide.lg_lstm_wide_create(48, 512, w, w, w, w, 0, None) == -1
    assert wide.lg_lstm_wide_load_device(None, w, w, w, w, None) == -1 and b"null" in err()
    assert wide.lg_lstm_wide_destroy(None) == -1 and b"null" in err()
    MB = 1 << 20
    assert wide.lg_lstm_wide_step(None, None, *([MB] * 2), None, *([MB] * 8), 32, None) == -1 and b"both handles" in err()

    class _Lstm(ctypes.Structure):                                 # struct lg_lstm_wide in host memory: the refusals below come before the launch
        _fields_ = [("num_in", ctypes.c_int32), ("hidden", ctypes.c_int32), ("ksteps", ctypes.c_int32), ("device", ctypes.c_int32),
                    ("d_wp", ctypes.c_void_p), ("d_bp", ctypes.c_void_p)]
    l = _Lstm(48, 512, 280, 0, None, None)
    h = ctypes.addressof(l)
    bufs = [1 * MB, 2 * MB, 3 * MB, 4 * MB]                        # h_in, c_in, h_out, c_out
    step = lambda la, lc, xa, xc, a, c, n: wide.lg_lstm_wide_step(la, lc, xa, xc, None, *a, *c, n, None)
    none4 = [None] * 4
    assert step(h, None, None, None, bufs, none4, 32) == -1 and b"actor memory" in err()
    assert step(None, h, None, None, none4, bufs, 32) == -1 and b"critic memory" in err()
    for k in range(4):
        b = list(bufs)
        b[k] = None
        assert step(h, None, 5 * MB, None, b, none4, 32) == -1
        assert step(None, h, None, 5 * MB, none4, b, 32) == -1
    for n in (0, -4):
        assert step(h, None, 5 * MB, None, bufs, none4, n) == -2 and b"num_envs" in err()
    for alias in ([1 * MB, 2 * MB, 1 * MB, 4 * MB], [1 * MB, 2 * MB, 3 * MB, 2 * MB], [1 * MB, 2 * MB, 2 * MB, 4 * MB], [1 * MB, 2 * MB, 3 * MB, 3 * MB]):
        assert step(h, None, 5 * MB, None, alias, none4, 32) == -2 and b"alias" in err(), alias
        assert step(None, h, None, 5 * MB, none4, alias, 32) == -2 and b"alias" in err(), alias
    l2 = _Lstm(48, 512, 280, 1, None, None)
    assert step(h, ctypes.addressof(l2), 5 * MB, 5 * MB, bufs, [6 * MB, 7 * MB, 8 * MB, 9 * MB], 32) == -2 and b"devices" in err()

    dims = lambda *d: (ctypes.c_int32 * 5)(*d)
    for d in ((544, 128, 128, 128, 12), (48, 128, 128, 128, 12), (0, 128, 128, 128, 12), (512, 544, 128, 128, 12), (512, 128, 544, 128, 12),
              (512, 128, 128, 544, 12), (512, 128, 128, 16, 12), (512, 128, 128, 128, 0), (512, 128, 128, 128, 17)):
        assert wide.lg_lstm_wide_actor_create(dims(*d), 0, ctypes.byref(out)) == -4 and not out.value, d
    assert wide.lg_lstm_wide_actor_create(None, 0, ctypes.byref(out)) == -1 and wide.lg_lstm_wide_actor_create(dims(512, 128, 128, 128, 12), 0, None) == -1
    assert wide.lg_lstm_wide_actor_load_device(None, None, None, None, None) == -1
    assert wide.lg_lstm_wide_actor_destroy(None) == -1
    assert wide.lg_lstm_wide_actor_act(None, MB, MB, MB, 32, 1, 1, None, 0, None) == -1

    class _Actor(ctypes.Structure):                                # struct lg_lstm_wide_actor in host memory
        _fields_ = [("dims", ctypes.c_int32 * 5), ("pad", ctypes.c_int32 * 5), ("device", ctypes.c_int32), ("max_width", ctypes.c_int32),
                    ("w_off", ctypes.c_size_t * 4), ("b_off", ctypes.c_size_t * 4), ("d_p", ctypes.c_void_p), ("d_std", ctypes.c_void_p)]
    a = _Actor()
    assert wide.lg_lstm_wide_actor_act(ctypes.addressof(a), None, MB, MB, 32, 1, 1, None, 0, None) == -1
    assert wide.lg_lstm_wide_actor_act(ctypes.addressof(a), MB, None, MB, 32, 1, 1, None, 0, None) == -1
    assert wide.lg_lstm_wide_actor_act(ctypes.addressof(a), MB, MB, None, 0, 1, 1, None, 0, None) == -2 and b"num_envs" in err()


def test_kernel_resource_rows_have_no_spill_and_fit_two_waves_per_simd():
    rows = [l.split() for l in open(RESOURCES) if not l.startswith("#")]
    assert len(rows) == len(KERNELS), rows
    for k in KERNELS:
        assert sum(bool(re.match(rf"_ZN2lg{len(k)}{k}E", r[0])) for r in rows) == 1, k
    for r in rows:
        f = dict(zip(r[1::2], r[2::2]))
        assert f["spill"] == "0" and f["scratch"] == "0", r
        assert int(f["VGPRs"]) + int(f["AGPRs"]) <= 256, r             # 512 threads: two waves per SIMD
    for other in os.listdir(CSRC):
        if other.startswith("kernel_resources") and other != os.path.basename(RESOURCES):
            assert "lstm_wide" not in open(os.path.join(CSRC, other)).read(), other


def test_lstm_unsupported_reason_with_and_without_wide():
    from legged_games_gym_amd.rl.recurrent_actor import lstm_unsupported_reason, wide_memory_would_help
    for h in (288, 320, 480, 512):
        rnn = nn.LSTM(input_size=48, hidden_size=h)
        assert "up to 256" in lstm_unsupported_reason(rnn) and str(h) in lstm_unsupported_reason(rnn)
        assert lstm_unsupported_reason(rnn, wide=True) is None and wide_memory_would_help(rnn)
    for h in (32, 256):
        rnn = nn.LSTM(input_size=48, hidden_size=h)
        assert lstm_unsupported_reason(rnn) is None and lstm_unsupported_reason(rnn, wide=True) is None and not wide_memory_would_help(rnn)
    for rnn, word in ((nn.LSTM(48, 544), "up to 512"), (nn.LSTM(48, 48), "up to 512"), (nn.LSTM(257, 512), "257"), (nn.GRU(48, 512), "GRU"),
                      (nn.LSTM(48, 512, num_layers=2), "2-layer")):
        assert word in lstm_unsupported_reason(rnn, wide=True), word
        assert not wide_memory_would_help(rnn)
    assert lstm_unsupported_reason(nn.GRU(48, 64)) == lstm_unsupported_reason(nn.GRU(48, 64), wide=True)


def test_the_runner_reads_the_key(capsys, monkeypatch):
    from legged_games_gym_amd.rl import OnPolicyRunner
    from legged_games_gym_amd.rl import recurrent_actor
    from legged_games_gym_amd.rl.actor_critic import ActorCriticRecurrent
    made = []

    class Fake:                                                    # stands in for the device objects: the key logic is what is tested here
        def __init__(self, ac, device, **kw):
            made.append(kw)
            self.wide = kw.get("wide", False)
    monkeypatch.setattr(recurrent_actor, "RecurrentFusedActor", Fake)
    ac = ActorCriticRecurrent(48, 48, 12, [32, 32, 32], [32, 32, 32], rnn_hidden_size=512)
    counter = types.SimpleNamespace(buf={"step_counter": None})
    loco = types.SimpleNamespace(_sim=counter, num_privileged_obs=None, num_envs=4, cfg=types.SimpleNamespace(seed=1))
    game = types.SimpleNamespace(ll_env=types.SimpleNamespace(_sim=counter), step_policy=lambda *a, **k: None, num_privileged_obs=None, num_envs=4,
                                 cfg=types.SimpleNamespace(seed=1), shared_actor_launch=lambda fused: False)

    def make(cfg, env, policy=ac):
        r = OnPolicyRunner.__new__(OnPolicyRunner)
        r.cfg, r.device, r.env, r.alg, r.num_steps_per_env = cfg, "cuda:0", env, types.SimpleNamespace(actor_critic=policy), 4
        capsys.readouterr()
        try:
            fused = r._make_fused_actor()
        except Exception as exc:                                   # (torch.zeros on cuda without a GPU, after the decision was taken)
            fused = exc
        return r, fused, capsys.readouterr().out

    _, fused, out = make({}, loco)                                 # without the key: today's message, and the key named
    assert fused is None and not made and "device LSTM cell unavailable" in out and "up to 256" in out and "torch policy in the rollout" in out
    assert "wide_memory" in out and out.count("\n") == 1
    _, fused, out = make({"wide_memory": True}, loco)
    assert made and made[-1]["wide"] is True and "unavailable" not in out
    del made[:]
    _, fused, out = make({"device_rollout": True}, game)
    assert fused is None and not made and "device rollout unavailable" in out and "512" in out and "generic VecEnv loop" in out
    assert "wide_memory" in out and out.count("\n") == 1
    _, fused, out = make({"device_rollout": True, "wide_memory": True}, game)
    assert made and made[-1]["wide"] is True and "unavailable" not in out
    del made[:]
    # a memory the key does not help either (544 units, GRU) keeps its reason and does not name the key
    for policy in (ActorCriticRecurrent(48, 48, 12, [32, 32, 32], [32, 32, 32], rnn_hidden_size=544),
                   ActorCriticRecurrent(48, 48, 12, [32, 32, 32], [32, 32, 32], rnn_type="gru", rnn_hidden_size=512)):
        for cfg in ({}, {"wide_memory": True}):
            _, fused, out = make(cfg, loco, policy)
            assert fused is None and not made and "device LSTM cell unavailable" in out and "wide_memory" not in out, out
    # 256 units: the key changes nothing that is said, and the wrapper decides that nothing wide is built
    narrow = ActorCriticRecurrent(48, 48, 12, [32, 32, 32], [32, 32, 32], rnn_hidden_size=256)
    _, fused, out = make({}, loco, narrow)
    assert made and made[-1]["wide"] is False and "unavailable" not in out


def _dec_cfg(units, **runner):
    return {"runner": dict(policy_class_name="ActorCriticRecurrent", device_rollout=True, **runner),
            "policy": dict(rnn_type="lstm", rnn_hidden_size=units, rnn_num_layers=1), "algorithm": {}}


def test_the_dec_runner_accepts_wide_memories_with_the_key_only():
    from legged_games_gym_amd.rl import DecGamePolicyRunner
    r = DecGamePolicyRunner.__new__(DecGamePolicyRunner)

    def check(units, **runner):
        cfg = _dec_cfg(units, **runner)
        r.cfg = cfg["runner"]
        return r._check_policy_class(cfg, "cuda:0")
    for units in (288, 320, 480, 512):
        with pytest.raises(ValueError, match=f"no device LSTM cell.*{units}.*up to 256.*no generic loop.*wide_memory"):
            check(units)
        assert check(units, wide_memory=True) is True
    assert check(256) is True and check(256, wide_memory=True) is True
    for units in (544, 48):
        with pytest.raises(ValueError, match="no device LSTM cell.*up to 512") as e:
            check(units, wide_memory=True)
        assert "wide_memory" not in str(e.value)
    with pytest.raises(ValueError, match="wide_memory.*opponent_pool_recurrent.*256 units"):
        check(512, wide_memory=True, opponent_pool_size=2, opponent_pool_recurrent=True)
    with pytest.raises(ValueError, match="wide_memory.*opponent_pool_recurrent.*256 units"):
        check(256, wide_memory=True, opponent_pool_size=2, opponent_pool_recurrent=True)
    assert check(256, opponent_pool_size=2, opponent_pool_recurrent=True) is True


def test_the_wrapper_marks_wide_only_above_256_units(monkeypatch):
    """``RecurrentFusedActor(wide=True)``: which handles it asks for, decided before any is made."""
    from legged_games_gym_amd.rl import recurrent_actor
    from legged_games_gym_amd.rl.actor_critic import ActorCriticRecurrent
    asked = []
    monkeypatch.setattr(recurrent_actor, "DeviceLstm", lambda rnn, device, wide=False: asked.append(("lstm", wide)) or types.SimpleNamespace(hidden=rnn.hidden_size, lib=None))
    monkeypatch.setattr(recurrent_actor, "DeviceLstmActor",
                        lambda ac, device, seed=1, step_counter=None, wide=False: asked.append(("actor", wide)) or types.SimpleNamespace(lib=None))
    for units, key, want in ((512, True, True), (288, True, True), (256, True, False), (64, True, False), (512, False, False)):
        del asked[:]
        ac = ActorCriticRecurrent(48, 48, 12, [32, 32, 32], [32, 32, 32], rnn_hidden_size=units)
        f = recurrent_actor.RecurrentFusedActor(ac, "cuda:0", wide=key)
        assert f.wide is want and asked == [("lstm", want), ("lstm", want), ("actor", want)], (units, key, asked)
    assert recurrent_actor.RecurrentFusedActor.recurrent is True


def test_the_flag_reaches_the_parser():
    from legged_games_gym_amd.utils import get_args
    assert get_args(["--task", "anymal_c_flat"]).wide_memory is False
    assert get_args(["--task", "anymal_c_flat", "--wide_memory"]).wide_memory is True
