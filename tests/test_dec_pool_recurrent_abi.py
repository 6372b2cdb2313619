"""The opponent pool for recurrent policies of ``dec_high_level_game`` without a GPU: the header's functions are
``capi.DEC_POOL_RECURRENT_SYMBOLS`` (include/legged_dec_pool_recurrent.h), a fifth library exports them and refuses bad arguments before
anything is allocated or launched, the struct sizes it sees, its kernel resource table, the pure stale-block rule and ``assign`` of
``rl.RecurrentOpponentPool`` on CPU tensors, and what ``DecGamePolicyRunner`` and ``DecHighLevelGame._recurrent_pair`` accept and refuse."""
import ctypes
import os
import re
import types

import pytest
import torch

from legged_games_gym_amd import capi
from tests.test_dec_game_recurrent_abi import MB, _declared, _Lstm, _LstmActor, _Policy, _train_cfg

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
CSRC = os.path.join(REPO, "legged_games_gym_amd", "csrc")
RESOURCES = os.path.join(CSRC, "kernel_resources_dec_pool_recurrent.txt")
OTHER_RESOURCES = ("kernel_resources.txt", "kernel_resources_game_recurrent.txt", "kernel_resources_dec_game_recurrent.txt", "kernel_resources_lstm_seq.txt")
HEADER = "legged_dec_pool_recurrent.h"
KERNELS = ("k_dec_pool_lstm_cell", "k_dec_pool_lstm_act")


@pytest.fixture(scope="module")
def libs():
    paths = (capi.dec_pool_recurrent_library_path(), capi.library_path(), capi.lstm_seq_library_path(), capi.game_recurrent_library_path(),
             capi.dec_game_recurrent_library_path())
    if not all(os.path.isfile(p) for p in paths):
        import __graft_entry__ as entry
        entry.build()
    return (capi.bind_dec_pool_recurrent(ctypes.CDLL(paths[0])),) + tuple(ctypes.CDLL(p) for p in paths[1:])


def test_header_symbol_list_matches_binding_and_is_disjoint_from_the_other_libraries():
    assert sorted(_declared(HEADER)) == sorted(capi.DEC_POOL_RECURRENT_SYMBOLS)
    assert {"lg_dec_rpool_create", "lg_dec_rpool_destroy", "lg_dec_rpool_query", "lg_dec_pool_lstm_step", "lg_dec_pool_lstm_act",
            "lg_dec_pool_recurrent_last_error", "lg_dec_pool_recurrent_sizeof"} == set(capi.DEC_POOL_RECURRENT_SYMBOLS)
    for other in (capi.ALL_SYMBOLS, capi.LSTM_SEQ_SYMBOLS, capi.GAME_RECURRENT_SYMBOLS, capi.DEC_GAME_RECURRENT_SYMBOLS):
        assert not set(capi.DEC_POOL_RECURRENT_SYMBOLS) & set(other)
    assert HEADER not in capi.ABI
    for header in list(capi.ABI) + ["legged_game_recurrent.h", "legged_lstm_sequence.h", "legged_dec_game_recurrent.h"]:
        assert not set(capi.DEC_POOL_RECURRENT_SYMBOLS) & set(_declared(header)), header


def test_the_fifth_library_exports_the_symbols_and_the_other_libraries_do_not(libs, monkeypatch):
    pool, *others = libs
    for sym in capi.DEC_POOL_RECURRENT_SYMBOLS:
        assert hasattr(pool, sym), sym
        for lib in others:
            assert not hasattr(lib, sym), (sym, lib._name)
    for sym in capi.DEC_GAME_RECURRENT_SYMBOLS + capi.GAME_RECURRENT_SYMBOLS + ["lg_lstm_step", "lg_dec_pool_act", "lg_dec_pool_create", "lg_lstm_seq_forward"]:
        assert not hasattr(pool, sym), sym                         # ... and it holds nothing of theirs
    assert len(pool.lg_dec_pool_lstm_act.argtypes) == 26 and len(pool.lg_dec_pool_lstm_step.argtypes) == 8 and len(pool.lg_dec_rpool_create.argtypes) == 6
    import __graft_entry__ as entry
    assert entry.DEC_POOL_REC_SOURCE == "lg_dec_pool_lstm_act.hip" and entry.DEC_POOL_REC_SOURCE not in entry.HIP_SOURCES
    assert os.path.basename(entry.DEC_POOL_REC_LIB) == "liblegged_dec_pool_recurrent.so" and os.path.basename(entry.DEC_POOL_REC_RESOURCES) == os.path.basename(RESOURCES)
    assert not any(os.path.basename(h) == HEADER for h in entry.HIP_HEADERS)
    # the library's staleness check reads every header its source includes, and both recurrent dec libraries read the shared one
    for source, headers in ((entry.DEC_POOL_REC_SOURCE, entry.DEC_POOL_REC_HEADERS), (entry.DEC_GAME_REC_SOURCE, entry.DEC_GAME_REC_HEADERS)):
        included = {os.path.basename(i) for i in re.findall(r'#include\s+"([^"]+)"', open(os.path.join(CSRC, source)).read())}
        assert included <= {os.path.basename(h) for h in headers}, (source, included)
        assert {"lg_lstm_cell_body.h", "lg_lstm_actor_body.h", "lg_dec_lstm_act.h"} <= included, source
    text = open(os.path.join(CSRC, entry.DEC_POOL_REC_SOURCE)).read()
    assert "lstm_cell_role(pool_lstm_role(" in text and "dec_lstm_actor_role<true>(pool_actor_args(" in text        # the shared bodies, not copies of them
    assert "dec_lstm_actor_role(const LstmActorArgs" not in text and "dec_lstm_actor_role(const LstmActorArgs" not in open(os.path.join(CSRC, entry.DEC_GAME_REC_SOURCE)).read()
    monkeypatch.setenv("LG_DEC_POOL_RECURRENT_LIB", "/nonexistent/liblegged_dec_pool_recurrent.so")
    assert capi.dec_pool_recurrent_library_path() == "/nonexistent/liblegged_dec_pool_recurrent.so"
    monkeypatch.setattr(capi.LIBRARIES["dec_pool_recurrent"], "handle", None)
    with pytest.raises(RuntimeError, match="not built"):
        capi.load_dec_pool_recurrent_library()


def test_struct_sizes_agree_with_the_binding_and_the_sibling_library(libs):
    pool, dec = libs[0], libs[4]
    for which in range(7):
        assert pool.lg_dec_pool_recurrent_sizeof(which) == dec.lg_dec_game_recurrent_sizeof(which) > 0, which
    for which, st in capi.DEC_POOL_RECURRENT_STRUCTS.items():
        assert pool.lg_dec_pool_recurrent_sizeof(which) == ctypes.sizeof(st), which
    assert pool.lg_dec_pool_recurrent_sizeof(3) == ctypes.sizeof(_Policy) and pool.lg_dec_pool_recurrent_sizeof(4) == ctypes.sizeof(_LstmActor)
    assert pool.lg_dec_pool_recurrent_sizeof(5) == ctypes.sizeof(_Lstm) and pool.lg_dec_pool_recurrent_sizeof(7) == ctypes.sizeof(capi.lg_dec_rpool_info) == 56
    assert pool.lg_dec_pool_recurrent_sizeof(8) == -1 and pool.lg_dec_pool_recurrent_sizeof(-1) == -1


def _member(role, units=64, hidden=(64, 64, 32), device=0):
    """A fake member of ``role`` (1 prey, 2 predator) in host memory: the shapes ``lg_lstm_create`` / ``lg_lstm_actor_create`` would give."""
    num_in, actions = (16, 4) if role == 1 else (3, 2)
    l = _Lstm(num_in=num_in, hidden=units, ksteps=(num_in + units + 1) // 2, device=device)
    a = _LstmActor()
    dims = [units, *hidden, actions]
    a.dims[:], a.pad[:] = dims, [(d + 31) // 32 * 32 for d in dims]
    a.device, a.max_width = device, max(a.pad)
    off = 0
    for i in range(4):
        a.w_off[i] = off
        off += a.pad[i + 1] * dims[i]
        a.b_off[i] = off
        off += a.pad[i + 1]
    return l, a


def test_pool_creation_refuses_bad_arguments_before_anything_is_allocated(libs):
    pool = libs[0]
    err = pool.lg_dec_pool_recurrent_last_error
    out = ctypes.c_void_p()

    def create(members, role=1, device=0, count=None, lstms=True, actors=True, result=True):
        ls = (ctypes.c_void_p * max(1, len(members)))(*[ctypes.addressof(m[0]) if m is not None and m[0] is not None else None for m in members])
        acs = (ctypes.c_void_p * max(1, len(members)))(*[ctypes.addressof(m[1]) if m is not None and m[1] is not None else None for m in members])
        rc = pool.lg_dec_rpool_create(ls if lstms else None, acs if actors else None, len(members) if count is None else count, role, device,
                                      ctypes.byref(out) if result else None)
        assert out.value is None                                    # nothing was created
        return rc

    good = [_member(1), _member(1), _member(1)]
    for kw in (dict(lstms=False), dict(actors=False), dict(result=False)):
        assert create(good, **kw) == -1 and b"null" in err(), kw
    assert create([good[0], None, good[2]]) == -1 and b"member 1 is null" in err()
    assert create([good[0], (good[1][0], None)]) == -1 and b"member 1 is null" in err()
    for count in (0, -1, 17):
        assert create(good, count=count) == -2 and b"count" in err(), count
    for role in (0, 3, -1):
        assert create(good, role=role) == -2 and b"role" in err(), role
    assert create(good, device=1) == -2 and b"another device" in err()
    assert create([good[0], _member(1, device=1)]) == -2 and b"member 1 lives on another device" in err()
    # a shape that is not the role's: a predator among preys, a prey pool asked to be a predator pool, an actor that does not sit on its memory
    assert create([good[0], _member(2)]) == -4 and b"member 1 is not a prey" in err()
    assert create(good, role=2) == -4 and b"member 0 is not a predator" in err()
    l, a = _member(1)
    a.dims[0] = 32
    assert create([(l, a)]) == -4 and b"not a prey" in err()
    # a shape that differs from member 0's: units, a hidden width, and nothing else
    assert create([good[0], _member(1, units=32)]) == -4 and b"member 1 differs" in err()
    assert create([good[0], good[1], _member(1, hidden=(64, 32, 32))]) == -4 and b"member 2" in err()
    assert pool.lg_dec_rpool_destroy(None) == -1 and pool.lg_dec_rpool_query(None, None) == -1 and b"null" in err()
    # every call above returned before the allocation; a valid call is not made with fake handles (tests/test_gpu_dec_pool_recurrent.py makes it)


class _RPool(ctypes.Structure):
    """``struct lg_dec_rpool`` (csrc/lg_dec_pool_lstm_act.hip) in host memory: what the launches read of a pool before they would launch."""
    _fields_ = [("d_table", ctypes.c_void_p), ("count", ctypes.c_int32), ("role", ctypes.c_int32), ("device", ctypes.c_int32), ("lstm", _Lstm), ("actor", _LstmActor)]


def _fake_pool(role, **kw):
    l, a = _member(role, **kw)
    p = _RPool(d_table=64 * MB, count=3, role=role, device=kw.get("device", 0))
    ctypes.memmove(ctypes.addressof(p.lstm), ctypes.addressof(l), ctypes.sizeof(l))
    ctypes.memmove(ctypes.addressof(p.actor), ctypes.addressof(a), ctypes.sizeof(a))
    return p


def test_pooled_cell_launch_refuses_bad_arguments_before_any_launch(libs):
    pool = libs[0]
    err = pool.lg_dec_pool_recurrent_last_error
    l = _Lstm(num_in=3, hidden=64, ksteps=34, device=0)
    prey_pool, pred_pool = _fake_pool(1), _fake_pool(2)
    role = lambda **kw: dict(dict(l=ctypes.addressof(l), x=1 * MB, h_in=2 * MB, c_in=3 * MB, h_out=4 * MB, c_out=5 * MB), **kw)

    def call(roles, n=64, pool_pred=None, slots_pred=None, pool_prey=None, slots_prey=None):
        arr = (capi.lg_dec_lstm_role * 4)()
        for slot, r in zip(arr, roles):
            for k, v in (r or {}).items():
                setattr(slot, k, v)
        return pool.lg_dec_pool_lstm_step(arr, ctypes.addressof(pool_pred) if pool_pred is not None else None, slots_pred,
                                          ctypes.addressof(pool_prey) if pool_prey is not None else None, slots_prey, None, n, None)

    assert pool.lg_dec_pool_lstm_step(None, None, None, None, None, None, 64, None) == -1 and b"null" in err()
    assert call([None] * 4) == -1 and b"null" in err()             # no present role and no pool
    assert call([role(), None, None, None], pool_prey=prey_pool) == -1 and b"block_slot" in err()        # a pool without its table
    assert call([role(), None, None, None], pool_pred=pred_pool) == -1 and b"block_slot" in err()
    for name in ("x", "h_in", "c_in", "h_out", "c_out"):           # a pooled role is present whatever its handle: its buffers are required
        assert call([None, None, role(l=None, **{name: None}), None], pool_prey=prey_pool, slots_prey=9 * MB) == -1 and b"null buffer of the prey actor" in err(), name
        assert call([role(**{name: None}), None, None, None]) == -1 and b"null buffer" in err(), name
    for n in (0, -3):
        assert call([None, None, role(l=None), None], n, pool_prey=prey_pool, slots_prey=9 * MB) == -2 and b"num_envs" in err(), n
    assert call([None, None, role(l=None), None], pool_prey=pred_pool, slots_prey=9 * MB) == -4 and b"other role" in err()
    assert call([role(l=None), None, None, None], pool_pred=prey_pool, slots_pred=9 * MB) == -4 and b"other role" in err()
    for alias in (dict(h_out=2 * MB), dict(c_out=3 * MB), dict(c_out=4 * MB)):
        assert call([None, None, role(l=None, **alias), None], pool_prey=prey_pool, slots_prey=9 * MB) == -2 and b"alias" in err(), alias
    assert call([role(), None, role(l=None), None], pool_prey=_fake_pool(1, device=1), slots_prey=9 * MB) == -2 and b"different devices" in err()
    assert call([None, None, role(l=None), None], pool_prey=_fake_pool(1, units=16), slots_prey=9 * MB) == -2 and b"shape" in err()
    # every call above returned before the launch; a valid call is not made with fake handles (tests/test_gpu_dec_pool_recurrent.py makes it)


def test_pooled_actor_launch_refuses_bad_arguments_before_any_launch(libs):
    pool = libs[0]
    err = pool.lg_dec_pool_recurrent_last_error
    pred, prey = _member(2, 256, (512, 256, 128))[1], _member(1, 256, (512, 256, 128))[1]
    prey_pool, pred_pool = _fake_pool(1, units=256, hidden=(512, 256, 128)), _fake_pool(2, units=256, hidden=(512, 256, 128))
    ll = _Policy()
    ll.dims[:], ll.tiles[:], ll.wide = [235, 512, 256, 128, 12], [15, 32, 16, 8], True
    P = capi.lg_dec_game_params()
    P.num_envs = 64
    full = {"command_prey": 1 * MB, "command_pred": 2 * MB, "ll_commands": 3 * MB}
    B = capi.dec_game_buffers(full)
    adr = lambda s: ctypes.addressof(s) if s is not None else None

    def call(pred=pred, prey=prey, ll=ll, pool_pred=None, slots_pred=None, pool_prey=None, slots_prey=None, P=P, B=B, h_pred=4 * MB, h_prey=5 * MB, pred_obs=6 * MB,
             prey_obs=7 * MB, ll_obs=8 * MB, ll_actions=9 * MB, mean_pred=10 * MB, mean_prey=11 * MB, seeds=(1, 2), out_pred=None, out_prey=None):
        return pool.lg_dec_pool_lstm_act(adr(pred), adr(prey), adr(ll), adr(pool_pred), slots_pred, adr(pool_prey), slots_prey, ctypes.byref(P) if P is not None else None,
                                         ctypes.byref(B) if B is not None else None, h_pred, h_prey, pred_obs, prey_obs, ll_obs, ll_actions, mean_pred, mean_prey,
                                         seeds[0], seeds[1], 1, None, 0, 0, ctypes.byref(out_pred) if out_pred is not None else None,
                                         ctypes.byref(out_prey) if out_prey is not None else None, None)

    for name in ("pred", "prey", "ll", "P", "B", "h_pred", "h_prey", "ll_obs", "ll_actions", "mean_pred", "mean_prey"):
        assert call(**{name: None}) == -1 and b"null" in err(), name
    assert call(pool_prey=prey_pool) == -1 and b"block_slot" in err() and call(pool_pred=pred_pool) == -1 and b"block_slot" in err()
    # with a pool the role's handle may be NULL: the next refusal is another one (equal seeds), not the null handle
    assert call(prey=None, pool_prey=prey_pool, slots_prey=12 * MB, seeds=(5, 5)) == -2 and b"must differ" in err()
    assert call(pred=None, pool_pred=pred_pool, slots_pred=12 * MB, seeds=(5, 5)) == -2 and b"must differ" in err()
    for missing in full:
        assert call(B=capi.dec_game_buffers({k: v for k, v in full.items() if k != missing})) == -1 and b"null" in err(), missing
    copy = capi.lg_dec_act_outputs()
    copy.obs_copy = 13 * MB
    assert call(pred_obs=None, out_pred=copy) == -1 and call(prey_obs=None, out_prey=copy) == -1 and b"null" in err()
    for n in (0, -5):
        P.num_envs = n
        assert call() == -2 and b"num_envs" in err(), n
    P.num_envs = 64
    assert call(pool_prey=pred_pool, slots_prey=12 * MB) == -4 and b"other role" in err()
    assert call(pool_pred=prey_pool, slots_pred=12 * MB) == -4 and b"other role" in err()
    wide = _fake_pool(1, units=256, hidden=(544, 256, 128))
    assert call(prey=None, pool_prey=wide, slots_prey=12 * MB) == -4 and b"32 .. 512" in err()           # the pool's shape, not the ignored handle's
    prey.dims[4] = 3
    assert call() == -4
    assert call(pool_prey=prey_pool, slots_prey=12 * MB, seeds=(5, 5)) == -2                               # (the ignored handle's shape is not read)
    prey.dims[4] = 4
    ll.tiles[0] = 11
    assert call() == -4 and b"235" in err()
    ll.tiles[0] = 15
    # every call above returned before the launch; a valid call is not made with fake handles (tests/test_gpu_dec_pool_recurrent.py makes it)


def test_kernel_resource_table_lists_exactly_the_two_kernels_without_spills_and_no_other_table_names_them():
    rows = [l for l in open(RESOURCES) if not l.startswith("#")]
    assert len(rows) == 2, rows
    names = sorted(r.split()[0] for r in rows)
    assert sorted(re.match(r"_ZN2lg\d+([a-z_]+?)ENS_", n).group(1) for n in names) == sorted(KERNELS), names
    for row in rows:
        f = dict(zip(row.split()[1::2], row.split()[2::2]))
        assert f["spill"] == "0" and f["scratch"] == "0", row
        assert int(f["VGPRs"]) + int(f["AGPRs"]) <= 256, row      # 512 threads: two waves per SIMD
    for other in OTHER_RESOURCES:
        text = open(os.path.join(CSRC, other)).read()
        for name in KERNELS:
            assert name not in text, (name, other)


# ----------------------------------------------------------------------------- the stale-block rule
def test_stale_blocks_on_hand_made_tables():
    from legged_games_gym_amd.rl.opponent_pool import stale_blocks
    T = lambda *v: torch.tensor(v, dtype=torch.int32)
    same = T(0, 1, 2, 1)
    assert stale_blocks(same, same, (), 3).tolist() == [False] * 4                                  # an unchanged slot is kept
    assert stale_blocks(same, T(0, 2, 2, 0), (), 3).tolist() == [False, True, False, True]            # a changed slot is zeroed
    assert stale_blocks(same, same, (1,), 3).tolist() == [False, True, False, True]                  # an overwritten member, its slot unchanged
    assert stale_blocks(same, same, (0,), 3).tolist() == [False] * 4                                # member 0 is never stale by being overwritten
    assert stale_blocks(same, T(1, 1, 2, 0), (0, 2), 3).tolist() == [True, False, True, True]
    assert stale_blocks(T(0, 5, -3, 2), T(0, 2, 0, 9), (), 3).tolist() == [False] * 4               # the kernels' clamp: 5 and 9 are member 2, -3 is member 0
    assert stale_blocks([0, 1], [0, 1], [1], 2).dtype == torch.bool
    with pytest.raises(ValueError):
        stale_blocks(T(0, 1), T(0, 1, 2), (), 3)
    with pytest.raises(ValueError):
        stale_blocks(same, same, (3,), 3)


class _CpuPool:
    """``RecurrentOpponentPool`` with nothing of the device under it: the members and the C-side pool are stand-ins, the live actor's state
    lives on the CPU.  ``assign`` / ``set_slots`` / ``push`` / ``load_state`` are the class's own."""

    def __new__(cls, n, capacity=2, units=4):
        from legged_games_gym_amd.rl import RecurrentOpponentPool

        class Pool(RecurrentOpponentPool):
            def _make_member(self, ac):
                return types.SimpleNamespace(ac=ac, sync_device=lambda: None)

            def _create_pool(self):
                return "pool"

            def _destroy_pool(self):
                pass
        module = lambda: torch.nn.Linear(2, 2)
        live = types.SimpleNamespace(ac=module(), device=torch.device("cpu"), seed=1, step_counter=None, num_envs=n, _flip=0,
                                     state_a=[tuple(torch.ones(n, units) for _ in range(2)) for _ in range(2)])
        return Pool(live, module, capacity, "prey", seed=3, num_envs=n)


def test_assign_zeroes_both_slots_of_exactly_the_stale_rows_on_cpu_tensors():
    from legged_games_gym_amd.rl import OpponentPool, RecurrentOpponentPool
    from legged_games_gym_amd.rl.opponent_pool import PoolBase
    assert issubclass(OpponentPool, PoolBase) and issubclass(RecurrentOpponentPool, PoolBase) and not issubclass(RecurrentOpponentPool, OpponentPool)
    assert RecurrentOpponentPool.is_opponent_pool and RecurrentOpponentPool.recurrent and not getattr(OpponentPool, "recurrent", False)
    n = 70                                                          # three blocks, the last of 6 rows
    pool = _CpuPool(n)
    live = pool.live
    tensors = [t for pair in live.state_a for t in pair]
    assert pool.handle == "pool" and pool.slot_table(n).tolist() == [0, 0, 0] and pool._flip == 0
    pool.assign()                                                   # no snapshot yet: all live, nothing changes, nothing is zeroed
    assert pool._slots_host.tolist() == [0, 0, 0] and all(bool((t == 1).all()) for t in tensors)
    assert pool.push(live.ac.state_dict(), pushed_at=0) == 1 and pool._marked == {1} and pool.filled == 1
    pool.set_slots([0, 1, 0])                                       # block 1 goes to member 1
    assert not pool._marked
    for t in tensors:
        assert bool((t[:32] == 1).all()) and bool((t[32:64] == 0).all()) and bool((t[64:] == 1).all())
        t.fill_(2.0)
    pool.set_slots([0, 1, 0])                                       # the same table, nothing overwritten: nothing is zeroed
    assert all(bool((t == 2).all()) for t in tensors)
    assert pool.push(live.ac.state_dict()) == 2 and pool.push(live.ac.state_dict()) == 1 and pool._marked == {1, 2}
    pool.set_slots([0, 1, 0])                                       # the same table, but member 1 was overwritten
    for t in tensors:
        assert bool((t[:32] == 2).all()) and bool((t[32:64] == 0).all()) and bool((t[64:] == 2).all())
        t.fill_(3.0)
    drawn = pool.assign(torch.Generator().manual_seed(5))           # a seeded deal: exactly the changed blocks
    changed = (drawn != torch.tensor([0, 1, 0], dtype=torch.int32)).repeat_interleave(32)[:n]
    for t in tensors:
        assert bool((t[changed] == 0).all()) and bool((t[~changed] == 3).all())
    # a checkpoint carries the table; loading marks every snapshot and deals the table again
    state = pool.state()
    assert torch.equal(state["slots"], pool._slots_host) and set(state) == {"filled", "next", "snapshots", "pushed_at", "member_totals", "slots"}
    fresh = _CpuPool(n)
    fresh.load_state(state)
    assert torch.equal(fresh._slots_host, pool._slots_host) and fresh.filled == 2 and not fresh._marked
    for t in (t for pair in fresh.live.state_a for t in pair):
        assert bool((t[(pool._slots_host != 0).repeat_interleave(32)[:n]] == 0).all())
    # a live actor without a state yet (allocated as zeros at its first step): nothing to zero, no error
    pool.live.num_envs = None
    pool.set_slots([2, 2, 2])
    with pytest.raises(ValueError, match="blocks"):
        pool.set_slots([0, 1])


# ----------------------------------------------------------------------------- the runner and the env
def test_runner_refusals_of_the_recurrent_pool_key_name_their_reason_and_build_nothing():
    from legged_games_gym_amd.rl import DecGamePolicyRunner
    env = types.SimpleNamespace(_outcome=None)
    cfg = _train_cfg(device_rollout=True, opponent_pool_size=2, opponent_pool_recurrent=True)
    cfg["runner"]["policy_class_name"] = "ActorCritic"
    with pytest.raises(ValueError, match="opponent_pool_recurrent with feed-forward policies"):
        DecGamePolicyRunner(env, cfg, log_dir=None, device="cuda:0")
    del cfg["runner"]["policy_class_name"]                         # (the default class is feed-forward too)
    with pytest.raises(ValueError, match="opponent_pool_recurrent with feed-forward policies"):
        DecGamePolicyRunner(env, cfg, log_dir=None, device="cuda:0")
    for size in (0, None):
        with pytest.raises(ValueError, match="opponent_pool_recurrent without an opponent pool.*opponent_pool_size"):
            DecGamePolicyRunner(env, _train_cfg(device_rollout=True, opponent_pool_size=size, opponent_pool_recurrent=True), log_dir=None, device="cuda:0")
    with pytest.raises(ValueError, match="opponent pool is feed-forward.*opponent_pool_recurrent"):
        DecGamePolicyRunner(env, _train_cfg(device_rollout=True, opponent_pool_size=2), log_dir=None, device="cuda:0")
    with pytest.raises(ValueError, match="opponent pool is feed-forward"):
        DecGamePolicyRunner(env, _train_cfg(device_rollout=True, opponent_pool_size=2, opponent_pool_recurrent=False), log_dir=None, device="cuda:0")
    with pytest.raises(ValueError, match="needs a GPU.*cpu"):      # with the key the other refusals still come first
        DecGamePolicyRunner(env, _train_cfg(device_rollout=True, opponent_pool_size=2, opponent_pool_recurrent=True), log_dir=None, device="cpu")


def test_the_command_line_flag_is_off_by_default_and_no_field_of_the_config_classes():
    from legged_games_gym_amd.scripts import train_dec_game
    args = train_dec_game._args(["--opponent_pool", "4", "--opponent_pool_recurrent", "--policy_class_name", "ActorCriticRecurrent"])
    assert args.opponent_pool == 4 and args.opponent_pool_recurrent is True
    assert train_dec_game._args([]).opponent_pool_recurrent is False


def test_recurrent_pair_accepts_a_recurrent_pool_and_still_refuses_the_two_old_cases():
    from legged_games_gym_amd.envs.a1_game.dec_high_level_game import DecHighLevelGame
    rec, ff = types.SimpleNamespace(recurrent=True), types.SimpleNamespace()
    rpool = types.SimpleNamespace(is_opponent_pool=True, recurrent=True, live=rec)
    pool = types.SimpleNamespace(is_opponent_pool=True, live=ff)
    assert DecHighLevelGame._recurrent_pair(rec, rec, None, rpool) is True and DecHighLevelGame._recurrent_pair(rec, rec, rpool, None) is True
    assert DecHighLevelGame._recurrent_pair(rec, rec, rpool, rpool) is True
    with pytest.raises(ValueError, match="pool is feed-forward"):
        DecHighLevelGame._recurrent_pair(rec, rec, None, pool)
    with pytest.raises(ValueError, match="pool is feed-forward"):
        DecHighLevelGame._recurrent_pair(rec, rec, rpool, pool)
    with pytest.raises(ValueError, match="or neither"):
        DecHighLevelGame._recurrent_pair(rec, ff)
    with pytest.raises(ValueError, match="or neither"):            # a recurrent pool next to a feed-forward learner is a mixed pair
        DecHighLevelGame._recurrent_pair(ff, rec, None, rpool)
    assert DecHighLevelGame._recurrent_pair(ff, ff, pool, None) is False
