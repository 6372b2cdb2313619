"""The shared GRU cell launch of dec_high_level_game (include/legged_dec_game_gru.h, liblegged_dec_game_gru.so) without a GPU: the header's
prototypes and structs are ``capi.DEC_GAME_GRU_ABI``, a library of its own exports them and refuses bad arguments before any launch,
``build()``'s lists, its kernel resource row, and what the runners, the scripts and the env do with the key ``dec_gru_shared``."""
import ctypes
import inspect
import os
import re
import types

import pytest

from legged_games_gym_amd import capi

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
CSRC = os.path.join(REPO, "legged_games_gym_amd", "csrc")
HEADER = "legged_dec_game_gru.h"
RESOURCES = os.path.join(CSRC, "dec_game_gru_kernel_resources.txt")
SEPARATE = "lg_lstm_actor_act x 2 + lg_dec_game_pre + lg_policy_act"
# substrings by which existing tests count kernel rows of csrc/kernel_resources.txt
COUNTED = ("lstm_wide", "k_dec_pre", "k_dec_post", "k_dec_act", "k_dec_outcome", "k_game_", "k_prey_act", "k_policy_act", "k_pool_act", "k_pursuer_post",
           "k_outcome_post", "k_member_outcome", "k_privileged_obs", "k_step", "k_physics")


def _header_text(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def _ctype(decl):
    """The ctypes type the binding uses for one C parameter or return type of this header."""
    decl = " ".join(decl.split())
    m = re.match(r"const (lg_dec_gru_role) \w+\[4\]$", decl)
    if m:
        return ctypes.POINTER(capi.lg_dec_gru_role)
    if decl.startswith("const char *"):
        return ctypes.c_char_p
    if "*" in decl:
        return ctypes.c_void_p
    return {"int32_t": ctypes.c_int32, "int": ctypes.c_int}[decl.split()[0]]


def test_header_prototypes_and_structs_match_the_binding():
    text = _header_text(os.path.join(REPO, "include", HEADER))
    protos = re.findall(r"^\s*((?:const\s+)?\w+\s*\*?)\s*(lg_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M)
    assert [name for _, name, _ in protos] == capi.DEC_GAME_GRU_SYMBOLS == ["lg_dec_gru_step", "lg_dec_game_gru_last_error", "lg_dec_game_gru_sizeof"]
    for ret, name, params in protos:
        want_args, want_ret = capi.DEC_GAME_GRU_ABI[name]
        params = [p for p in (q.strip() for q in params.split(",")) if p and p != "void"]
        assert [_ctype(p) for p in params] == list(want_args), name
        assert _ctype(ret + " f") is want_ret, name
    # the role struct, field for field; the handle's layout (csrc/lg_gru.h) and its static_assert
    body = re.search(r"typedef struct lg_dec_gru_role \{(.*?)\} lg_dec_gru_role;", text, flags=re.S).group(1)
    fields = [n for decl in body.split(";") for n in re.findall(r"\*\s*(\w+)", decl)]
    assert fields == [n for n, _ in capi.lg_dec_gru_role._fields_] == ["l", "x", "h_in", "h_out"]
    assert all(t is ctypes.c_void_p for _, t in capi.lg_dec_gru_role._fields_)
    handle = _header_text(os.path.join(CSRC, "lg_gru.h"))
    body = re.search(r"struct lg_gru \{(.*?)\};", handle, flags=re.S).group(1)
    assert re.findall(r"\b(\w+)\s*[,;]", body) == [n for n, _ in capi.lg_gru_handle._fields_]
    assert int(re.search(r"static_assert\(sizeof\(lg_gru\) == (\d+)", handle).group(1)) == ctypes.sizeof(capi.lg_gru_handle) == 32
    assert capi.DEC_GAME_GRU_STRUCTS == {0: capi.lg_gru_handle, 1: capi.lg_dec_gru_role}
    # the constants are the GRU cell's: the header takes them from legged_recurrent_gru.h and defines none of its own
    raw = open(os.path.join(REPO, "include", HEADER)).read()
    assert '#include "legged_recurrent_gru.h"' in raw and re.findall(r"#define (\w+) ", raw) == []
    assert "67 584" in raw and 2 * ((capi.LG_GRU_MAX_IN + capi.LG_GRU_MAX_HIDDEN) // 2) * 33 * 4 == 67584
    for other in (capi.ALL_SYMBOLS, capi.LSTM_SEQ_SYMBOLS, capi.GAME_RECURRENT_SYMBOLS, capi.DEC_GAME_RECURRENT_SYMBOLS, capi.DEC_POOL_RECURRENT_SYMBOLS,
                  capi.DEC_GAME_PRIVILEGED_SYMBOLS, capi.LSTM_WIDE_SYMBOLS, capi.GRU_SYMBOLS):
        assert not set(capi.DEC_GAME_GRU_SYMBOLS) & set(other)
    assert HEADER not in capi.ABI


def test_build_lists_name_the_source_the_headers_and_the_resources_file():
    import __graft_entry__ as entry
    assert entry.DEC_GAME_GRU_SOURCE == "lg_dec_gru.hip" and entry.DEC_GAME_GRU_SOURCE not in entry.HIP_SOURCES
    assert os.path.basename(entry.DEC_GAME_GRU_LIB) == "liblegged_dec_game_gru.so" == os.path.basename(capi.dec_game_gru_library_path())
    assert entry.DEC_GAME_GRU_RESOURCES == RESOURCES
    assert {os.path.basename(h) for h in entry.DEC_GAME_GRU_OWN_HEADERS} == {"lg_gru.h", HEADER}
    included = {os.path.basename(i) for i in re.findall(r'#include\s+"([^"]+)"', open(os.path.join(CSRC, entry.DEC_GAME_GRU_SOURCE)).read())}
    assert included | {"legged_recurrent_gru.h"} == {os.path.basename(h) for h in entry.DEC_GAME_GRU_HEADERS}, included      # (the public header includes that one)
    for h in entry.DEC_GAME_GRU_HEADERS:
        assert os.path.isfile(h if os.path.isabs(h) else os.path.join(CSRC, h)), h
    assert not any(os.path.basename(h) in ("lg_gru.h", HEADER) for h in entry.HIP_HEADERS)      # the main library is not stale when they change
    assert "lg_gru.h" in entry.GRU_HEADERS and '#include "lg_gru.h"' in open(os.path.join(CSRC, entry.GRU_SOURCE)).read()
    assert "struct lg_gru {" not in open(os.path.join(CSRC, entry.GRU_SOURCE)).read()
    # build() writes that resources file, looks those symbols up and reports that library: through the library's row of the table
    spec = next(s for s in entry.LIBS if s.key == "dec_game_gru")
    assert (spec.resources, spec.symbols, spec.target) == (entry.DEC_GAME_GRU_RESOURCES, "DEC_GAME_GRU_SYMBOLS", entry.DEC_GAME_GRU_LIB)
    assert set(spec.checks) == {"no_spill", "two_waves"}
    source = inspect.getsource(entry.build)
    assert source.count("for spec in LIBS:") == 2 and "_check_resources(spec" in source and "getattr(capi, spec.symbols)" in source
    assert re.search(r"\[build\] ok:.*spec\.target for spec in LIBS", source)
    assert "_write_resources(table, spec.resources)" in inspect.getsource(entry._check_resources)


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(capi.dec_game_gru_library_path()):
        import __graft_entry__ as entry
        entry.build()
    return capi.bind_dec_game_gru(ctypes.CDLL(capi.dec_game_gru_library_path()))


def test_the_library_exports_the_symbols_sizes_its_structs_and_fails_loudly_when_absent(lib, monkeypatch):
    for sym in capi.DEC_GAME_GRU_SYMBOLS:
        assert hasattr(lib, sym), sym
    for other in (capi.gru_library_path(), capi.library_path(), capi.dec_game_recurrent_library_path()):
        if os.path.isfile(other):
            assert not any(hasattr(ctypes.CDLL(other), sym) for sym in capi.DEC_GAME_GRU_SYMBOLS), other
    assert (lib.lg_dec_game_gru_sizeof(0), lib.lg_dec_game_gru_sizeof(1), lib.lg_dec_game_gru_sizeof(2), lib.lg_dec_game_gru_sizeof(-1)) == (32, 32, -1, -1)
    monkeypatch.setenv("LG_DEC_GAME_GRU_LIB", "/nonexistent/liblegged_dec_game_gru.so")
    assert capi.dec_game_gru_library_path() == "/nonexistent/liblegged_dec_game_gru.so"
    monkeypatch.setattr(capi.LIBRARIES["dec_game_gru"], "handle", None)
    with pytest.raises(RuntimeError, match="not built; run"):
        capi.load_dec_game_gru_library()
    with pytest.raises(RuntimeError, match="not built; run"):
        capi.dec_gru_step([None] * 4, None, 1)


def test_bad_arguments_are_refused_before_any_launch(lib):
    """Handles in host memory and addresses that are never read: every call below is refused for its arguments, before the library
    makes its first HIP call (``call`` asserts the code), so nothing here reaches a device whether or not one is visible."""
    err = lib.lg_dec_game_gru_last_error
    MB = 1 << 20
    made = [capi.lg_gru_handle(I, H, (I + H + 1) // 2, 0, None, None) for I, H in ((3, 64), (3, 32), (16, 64), (16, 96))]
    names = (b"predator actor", b"predator critic", b"prey actor", b"prey critic")

    def call(edit=None, n=33, present=(0, 1, 2, 3)):
        roles = [[ctypes.addressof(made[r]), (4 * r + 1) * MB, (4 * r + 2) * MB, (4 * r + 3) * MB] if r in present else None for r in range(4)]
        if edit:
            edit(roles)
        rc = lib.lg_dec_gru_step(capi.dec_gru_roles(roles), None, n, None)
        assert rc in (-1, -2), rc                                   # a refusal of the arguments: neither a launch (0) nor a HIP call (-10)
        return rc, err()

    assert lib.lg_dec_gru_step(None, None, 33, None) == -1 and b"null roles" in err()
    rc, text = call(present=())
    assert rc == -1 and b"all four handles are null" in text
    for r in range(4):
        for field in (1, 2, 3):
            rc, text = call(lambda roles: roles[r].__setitem__(field, None))
            assert rc == -1 and b"null buffer" in text and names[r] in text, (r, field, text)
            rc, text = call(lambda roles: roles[r].__setitem__(field, None), present=(r,))
            assert rc == -1 and names[r] in text, (r, field, text)
        rc, text = call(lambda roles: roles[r].__setitem__(3, roles[r][2]))
        assert rc == -2 and b"alias" in text and names[r] in text, (r, text)
        for n in (0, -4):
            rc, text = call(n=n, present=(r,))
            assert rc == -2 and b"num_envs" in text
    elsewhere = capi.lg_gru_handle(16, 96, 56, 1, None, None)
    rc, text = call(lambda roles: roles[3].__setitem__(0, ctypes.addressof(elsewhere)))
    assert rc == -2 and b"different devices" in text
    def alone_and_aliased(roles):                                  # alone it is on one device: the refusal is the aliasing's, still before any launch
        roles[3][0], roles[3][3] = ctypes.addressof(elsewhere), roles[3][2]
    rc, text = call(alone_and_aliased, present=(3,))                # (a valid call is never made with handles in host memory)
    assert rc == -2 and b"alias" in text and b"devices" not in text
    odd = capi.lg_gru_handle(16, 288, 152, 0, None, None)          # a shape lg_gru_create does not make never sizes a launch
    rc, text = call(lambda roles: roles[1].__setitem__(0, ctypes.addressof(odd)))
    assert rc == -2 and b"outside what lg_gru_create makes" in text and names[1] in text
    with pytest.raises(ValueError, match="four roles"):
        capi.dec_gru_roles([None] * 5)


def test_kernel_resource_row_is_the_one_kernel_without_spill():
    rows = [l.split() for l in open(RESOURCES) if not l.startswith("#")]
    assert len(rows) == 1 and re.match(r"_ZN2lg14k_dec_gru_cellE", rows[0][0]), rows
    f = dict(zip(rows[0][1::2], rows[0][2::2]))
    assert f["spill"] == "0" and f["scratch"] == "0", rows[0]
    assert int(f["VGPRs"]) + int(f["AGPRs"]) <= 256, rows[0]            # 512 threads: two waves per SIMD
    assert not any(word in rows[0][0] for word in COUNTED), rows[0]     # the name stays out of the other tables' row counts
    for other in os.listdir(CSRC):                                      # ... and no other table lists it
        if other.endswith(".txt") and "kernel_resources" in other and other != os.path.basename(RESOURCES):
            assert "k_dec_gru_cell" not in open(os.path.join(CSRC, other)).read(), other
    design = open(os.path.join(REPO, "DESIGN.md")).read()              # the figures DESIGN.md quotes are the table's
    assert f"{f['VGPRs']} VGPRs, spill 0, occupancy {f['occupancy']}" in design


# ---------------------------------------------------------------------------------------------------------------- the key dec_gru_shared
def test_the_flag_is_parsed_and_the_scripts_set_the_runner_key(monkeypatch):
    from legged_games_gym_amd.utils import get_args
    assert get_args(["--task", "anymal_c_flat"]).dec_gru_shared is False
    assert get_args(["--task", "anymal_c_flat", "--dec_gru_shared"]).dec_gru_shared is True
    scripts = os.path.join(REPO, "legged_games_gym_amd", "scripts")
    for name in ("train_dec_game.py", "play_dec_game.py"):
        assert re.search(r"runner\.dec_gru_shared = True", open(os.path.join(scripts, name)).read()), name
    # crossplay_dec_game hands its own args to play_dec_game's DecEvaluation, whose constructor sets both keys from them
    import ast
    tree = ast.parse(open(os.path.join(scripts, "crossplay_dec_game.py")).read())
    assert any(isinstance(n, ast.ImportFrom) and n.module == "play_dec_game" and n.level == 1 and "DecEvaluation" in [a.name for a in n.names] for n in tree.body)
    crossplay = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "crossplay")
    assert crossplay.args.args[0].arg == "args"
    made = [n for n in ast.walk(crossplay) if isinstance(n, ast.Call) and getattr(n.func, "id", None) == "DecEvaluation"]
    assert len(made) == 1 and [getattr(a, "id", None) for a in made[0].args] == ["args"] and not made[0].keywords
    assert not any(isinstance(t, ast.Name) and t.id == "args" for n in ast.walk(crossplay) if isinstance(n, ast.Assign) for t in n.targets)      # never rebound
    play = ast.parse(open(os.path.join(scripts, "play_dec_game.py")).read())
    init = next(f for c in play.body if isinstance(c, ast.ClassDef) and c.name == "DecEvaluation" for f in c.body if getattr(f, "name", "") == "__init__")
    body = ast.unparse(init).replace("'", '"')
    assert init.args.args[1].arg == "args" and 'getattr(args, "dec_gru_shared", False)' in body and "runner.dec_gru_shared = True" in body
    helpers = open(os.path.join(REPO, "legged_games_gym_amd", "utils", "helpers.py")).read()
    assert re.search(r'"--device_gru".*?--dec_gru_shared.*?"--dec_gru_shared"', helpers, flags=re.S)      # the --device_gru help names the new key


def test_the_key_is_no_config_field():
    from legged_games_gym_amd.envs import a1_game, task_registry
    from legged_games_gym_amd.utils.helpers import class_to_dict
    a1_game.register_dec()
    try:
        env_cfg, train_cfg = task_registry.get_cfgs("dec_high_level_game")
        for cfg in (env_cfg, train_cfg):
            assert "dec_gru_shared" not in repr(class_to_dict(cfg))
        train_cfg.runner.dec_gru_shared = True                        # what the scripts do: an attribute on this registration
        try:
            assert class_to_dict(train_cfg)["runner"]["dec_gru_shared"] is True
        finally:
            del train_cfg.runner.dec_gru_shared
        assert "dec_gru_shared" not in vars(type(train_cfg.runner))
    finally:
        a1_game.unregister_dec()


def _dec_cfg(units, kind="gru", **runner):
    return {"runner": dict(policy_class_name="ActorCriticRecurrent", device_rollout=True, **runner),
            "policy": dict(rnn_type=kind, rnn_hidden_size=units, rnn_num_layers=1), "algorithm": {}}


def test_the_dec_runner_refuses_the_key_without_gru_memories_on_the_device():
    from legged_games_gym_amd.rl import DecGamePolicyRunner
    r = DecGamePolicyRunner.__new__(DecGamePolicyRunner)

    def check(units, kind="gru", **runner):
        cfg = _dec_cfg(units, kind, **runner)
        r.cfg = cfg["runner"]
        return r._check_policy_class(cfg, "cuda:0")
    both = "dec_gru_shared.*rnn_type 'gru'.*device_gru"
    with pytest.raises(ValueError, match=both) as first:
        check(64, dec_gru_shared=True)                                # the key without device_gru
    with pytest.raises(ValueError, match=both) as second:
        check(64, "lstm", dec_gru_shared=True, device_gru=True)       # the key with an LSTM
    assert str(first.value) == str(second.value)
    with pytest.raises(ValueError, match=both):
        check(64, "lstm", dec_gru_shared=True)
    for units in (32, 64, 256):
        assert check(units, device_gru=True, dec_gru_shared=True) is True
    # device_gru with a recurrent pool: today's refusal with and without the key
    texts = []
    for keys in ({}, {"dec_gru_shared": True}):
        with pytest.raises(ValueError, match="device_gru.*opponent_pool_recurrent.*lg_lstm handles") as e:
            check(64, device_gru=True, opponent_pool_size=2, opponent_pool_recurrent=True, **keys)
        texts.append(str(e.value))
    assert texts[0] == texts[1]
    with pytest.raises(ValueError, match="device_gru.*no device GRU cell.*288.*up to 256"):
        check(288, device_gru=True, dec_gru_shared=True)              # above 256 units: the GRU cell's own refusal
    # without the key nothing moved
    assert check(64, device_gru=True) is True and check(64, "lstm", device_gru=True) is True
    with pytest.raises(ValueError, match="no device LSTM cell for a GRU memory"):
        check(64)


def test_the_wrapper_and_the_runner_carry_the_key(monkeypatch, capsys):
    from legged_games_gym_amd.rl import OnPolicyRunner, recurrent_actor
    from legged_games_gym_amd.rl.actor_critic import ActorCriticRecurrent
    sig = inspect.signature(recurrent_actor.RecurrentFusedActor.__init__)
    assert sig.parameters["shared_gru"].default is False and recurrent_actor.RecurrentFusedActor.shared_gru is False
    monkeypatch.setattr(recurrent_actor, "DeviceGru", lambda rnn, device: types.SimpleNamespace(hidden=rnn.hidden_size, lib="gru-lib"))
    monkeypatch.setattr(recurrent_actor, "DeviceLstm", lambda rnn, device, wide=False: types.SimpleNamespace(hidden=rnn.hidden_size, lib="main"))
    monkeypatch.setattr(recurrent_actor, "DeviceLstmActor", lambda ac, device, seed=1, step_counter=None, wide=False: types.SimpleNamespace(lib=None))
    policy = lambda **kw: ActorCriticRecurrent(3, 3, 2, [32, 32, 32], [32, 32, 32], rnn_hidden_size=64, **kw)
    gru, lstm = policy(rnn_type="gru"), policy()
    make = recurrent_actor.RecurrentFusedActor
    assert make(gru, "cuda:0", gru=True, shared_gru=True).shared_gru is True
    assert make(gru, "cuda:0", gru=True).shared_gru is False
    assert make(lstm, "cuda:0", gru=True, shared_gru=True).shared_gru is False       # true only when gru is true as well
    assert make(lstm, "cuda:0", shared_gru=True).shared_gru is False

    made = []

    class _Fake:
        def __init__(self, ac, device, **kw):
            made.append(kw)
    monkeypatch.setattr(recurrent_actor, "RecurrentFusedActor", _Fake)
    counter = types.SimpleNamespace(buf={"step_counter": None})
    view = types.SimpleNamespace(ll_env=types.SimpleNamespace(_sim=counter), step_policy=lambda *a, **k: None, num_privileged_obs=None, num_envs=4,
                                 cfg=types.SimpleNamespace(seed=1), shared_actor_launch=lambda fused: None)

    def built(cfg, ac):
        r = OnPolicyRunner.__new__(OnPolicyRunner)
        r.cfg, r.device, r.env, r.alg, r.num_steps_per_env = dict(cfg, device_rollout=True), "cuda:0", view, types.SimpleNamespace(actor_critic=ac), 4
        del made[:]
        try:
            r._make_fused_actor()
        except Exception:                                             # (torch.zeros on cuda without a GPU, after the actor was made)
            pass
        return made[-1]
    assert built({"device_gru": True, "dec_gru_shared": True}, gru) .get("shared_gru") is True
    assert "shared_gru" not in built({"device_gru": True}, gru)
    assert "shared_gru" not in built({"device_gru": True, "dec_gru_shared": True}, lstm) and "gru" not in made[-1]
    assert "unavailable" not in capsys.readouterr().out


# ---------------------------------------------------------------------------------------------------------------- the env's choice of launches
def _env():
    from legged_games_gym_amd.envs.a1_game.dec_high_level_game import DecHighLevelGame
    return DecHighLevelGame.__new__(DecHighLevelGame)


def _stub(gru=True, shared=False, precision=1):
    return types.SimpleNamespace(recurrent=True, wide=False, gru=gru, shared_gru=shared,
                                 lib=types.SimpleNamespace(lg_mlp_wide_set_precision=lambda mode: precision))


def test_recurrent_launches_without_the_key_and_for_a_mixed_pair_are_todays(capsys):
    for pair in ((_stub(), _stub()), (_stub(shared=True), _stub()), (_stub(), _stub(shared=True)), (_stub(shared=True), _stub(gru=False)),
                 (_stub(gru=False), _stub(shared=True))):
        env = _env()
        assert env._recurrent_launches(*pair) == (None, False)
        out = capsys.readouterr().out
        assert out == f"[{env.TASK}] recurrent actor launch unavailable (GRU memory); {SEPARATE}\n", out
        assert env._recurrent_launches(*pair) == (None, False) and capsys.readouterr().out == ""      # said once
        assert env._recurrent_launches(*pair, say=False) == (None, False)
    env = _env()                                                      # a pool next to GRU actors: today's answer with the key, too
    assert env._recurrent_launches(_stub(shared=True), _stub(shared=True), pooled=True) == (None, False)
    assert "pooled recurrent actor launch unavailable (GRU memory)" in capsys.readouterr().out


def test_recurrent_launches_of_a_shared_pair(lib, monkeypatch, capsys):
    pair = (_stub(shared=True), _stub(shared=True))
    monkeypatch.setattr(capi.LIBRARIES["dec_game_gru"], "handle", None)
    env = _env()
    if not os.path.isfile(capi.dec_game_recurrent_library_path()):
        import __graft_entry__ as entry
        entry.build()
    got, shared = env._recurrent_launches(*pair)
    assert got is capi.load_dec_game_gru_library() and shared is True and capsys.readouterr().out == ""
    # wide precision 0: the cell launch stays shared, the actors take the separate launches with the existing line
    zero = (_stub(shared=True, precision=0), _stub(shared=True, precision=0))
    got, shared = env._recurrent_launches(*zero)
    assert got is capi.load_dec_game_gru_library() and shared is False
    assert capsys.readouterr().out == f"[{env.TASK}] recurrent actor launch unavailable (wide precision 0); {SEPARATE}\n"
    # without liblegged_dec_game_recurrent.so: likewise
    monkeypatch.setattr(capi.LIBRARIES["dec_game_recurrent"], "handle", None)
    monkeypatch.setenv("LG_DEC_GAME_RECURRENT_LIB", "/nonexistent/liblegged_dec_game_recurrent.so")
    env = _env()
    got, shared = env._recurrent_launches(*pair)
    out = capsys.readouterr().out
    assert got is capi.load_dec_game_gru_library() and shared is False and out.count("\n") == 1 and "liblegged_dec_game_recurrent.so" in out and SEPARATE in out
    # without the new library: everything separate, one line that names it
    monkeypatch.setattr(capi.LIBRARIES["dec_game_gru"], "handle", None)
    monkeypatch.setenv("LG_DEC_GAME_GRU_LIB", "/nonexistent/liblegged_dec_game_gru.so")
    env = _env()
    assert env._recurrent_launches(*pair) == (None, False)
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "liblegged_dec_game_gru.so" in out and SEPARATE in out, out
    assert env._recurrent_launches(*pair) == (None, False) and capsys.readouterr().out == ""
