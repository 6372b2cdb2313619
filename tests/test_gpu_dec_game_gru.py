"""The shared cell launch of GRU policies on ``dec_high_level_game`` (``lg_dec_gru_step``, include/legged_dec_game_gru.h: k_dec_gru_cell)
against ``lg_gru_step`` with each role alone (bit for bit) and against the float64 restatement of ``tests/gru_ref.py``, its error codes,
and the runner key ``dec_gru_shared`` through ``DecHighLevelGame`` (eager and captured) and ``DecGamePolicyRunner``.

The bars are the project's own: ``torch.equal`` where the contract says bit-identical, ``TOL = 2e-5`` of ``max(1, max |want|)`` against
float64 (the bar of ``tests/test_gpu_recurrent_gru.py``; a GRU's outputs are convex combinations of tanh values and ``h_in``, so with
``|h_in| <= 1`` the scale is 1)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests.gru_ref import gru_params64, gru_step64

pytestmark = pytest.mark.gpu
TOL = 2e-5
DEV = "cuda:0"
EXTRA = 5                    # NaN guard rows behind row N of every input and output
# (num_in, hidden) of predator actor / predator critic / prey actor / prey critic: the task's input widths, one / two / three waves of units
ROLES = ((3, 64), (3, 32), (16, 64), (16, 96))
NAMES = ("pred_actor", "pred_critic", "prey_actor", "prey_critic")

_cache = {}


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _np64(t):
    return t.detach().cpu().double().numpy()


def _guarded(values):
    """``values`` [N, W] on the device as a view of a buffer whose rows behind N are NaN."""
    n, w = values.shape
    full = torch.full((n + EXTRA, w), float("nan"), device=DEV)
    full[:n] = values.to(DEV)
    return full[:n]


def _padded(n, H):
    """An output buffer of ``n`` rows, NaN throughout, with NaN sentinels behind it: ``(whole buffer, the n rows)``."""
    t = torch.full((n + EXTRA, H), float("nan"), device=DEV)
    return t, t[:n]


def _cell(I, H, seed):
    """``(nn.GRU, DeviceGru)`` of one shape, made once per module."""
    from legged_games_gym_amd.rl.recurrent_actor import DeviceGru
    key = ("cell", I, H, seed)
    if key not in _cache:
        torch.manual_seed(seed)
        rnn = nn.GRU(I, H).to(DEV)
        _cache[key] = (rnn, DeviceGru(rnn, DEV))
    return _cache[key]


def _inputs(shapes, n, seed, first=1):
    """Per role ``(x, h_in)`` with a non-zero state, and reset flags on every third row from row ``first`` (1: row 0 stays live, so a
    one-row launch has no reset row; 0: row 0 is reset)."""
    gen = torch.Generator().manual_seed(seed)
    xs = [_guarded((torch.rand(n, I, generator=gen) * 2.0 - 1.0) * 3.0) for I, _ in shapes]
    hs = [_guarded(torch.rand(n, H, generator=gen) * 2.0 - 1.0) for _, H in shapes]
    reset = (torch.arange(n) % 3 == first).to(torch.uint8).to(DEV)
    return xs, hs, reset


def _alone(cell, x, h, reset):
    """``lg_gru_step`` with this role alone (the actor slot of that launch) into a fresh guarded output."""
    from legged_games_gym_amd import capi
    from legged_games_gym_amd.rl.recurrent_actor import gru_step
    n, H = h.shape
    full, ho = _padded(n, H)
    gru_step(capi.load_gru_library(), cell, None, x, None, reset, h, ho, None, None, n, _stream())
    torch.cuda.synchronize()
    assert torch.isnan(full[n:]).all()
    return ho


def _shared(cells, xs, hs, reset, n, present):
    """One ``lg_dec_gru_step`` of the roles in ``present``; returns per role ``(whole output buffer, its n rows)``, NaN where nothing wrote."""
    from legged_games_gym_amd import capi
    outs = [_padded(n, h.shape[1]) for h in hs]
    roles = [(cells[r].handle, xs[r].data_ptr(), hs[r].data_ptr(), outs[r][1].data_ptr()) if r in present else None for r in range(len(cells))]
    roles += [None] * (4 - len(roles))
    capi.dec_gru_step(roles, None if reset is None else reset.data_ptr(), n, _stream())
    torch.cuda.synchronize()
    return outs


def _check_roles(shapes, n, seed, tag, slots=None, first=1):
    """All of ``shapes`` in one launch (role r in slot ``slots[r]``): every role bit-identical to that role alone and within TOL of float64,
    every guard NaN."""
    slots = list(range(len(shapes))) if slots is None else slots
    made = [_cell(I, H, 11 + r) for r, (I, H) in enumerate(shapes)]
    xs, hs, reset = _inputs(shapes, n, seed, first)
    by_slot = {s: r for r, s in enumerate(slots)}
    pick = lambda seq: [seq[by_slot[s]] if s in by_slot else seq[0] for s in range(4)]
    outs = _shared(pick([c for _, c in made]), pick(xs), pick(hs), reset, n, set(slots))
    assert int(reset.sum()) > 0 or (n == 1 and first == 1)
    for r, (rnn, cell) in enumerate(made):
        full, got = outs[slots[r]]
        alone = _alone(cell, xs[r], hs[r], reset)
        want = gru_step64(gru_params64(rnn), _np64(xs[r]), _np64(hs[r]), reset.cpu().numpy())
        err, scale = np.abs(_np64(got) - want).max(), max(1.0, np.abs(want).max())
        print(f"[observed] {tag} role {r} {shapes[r]} n={n}: err {err:.3e} = {err / (TOL * scale):.3f} of the bar")
        assert bool(torch.isfinite(got).all()) and torch.equal(got, alone), (tag, r, n)
        assert err < TOL * scale, (tag, r, n, err)
        assert torch.isnan(full[n:]).all(), (tag, r, n)
    for s in range(4):
        if s not in by_slot:
            assert torch.isnan(outs[s][0]).all(), (tag, s)
    return outs


# ---------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("n,first", [(1, 1), (1, 0), (33, 1), (64, 1)], ids=["1", "1-reset", "33", "64"])
def test_four_roles_in_one_launch_equal_each_role_alone_and_float64(n, first):
    """One row, live and (a second case) reset; two workgroups per role with one live row in the second; two full workgroups.  Roles of
    one, two and three waves share a launch sized for three."""
    outs = _check_roles(ROLES, n, 100 + n, "four roles", first=first)
    if (n, first) == (1, 0):                                        # the reset row started from h = 0: h_in does not reach the output
        again = _check_roles(ROLES, n, 100 + n, "four roles, reset", first=first)
        assert all(torch.equal(a[1], b[1]) for a, b in zip(outs, again))


def test_every_pattern_of_present_roles():
    """All 15 non-empty sets of present roles at 33 rows: a present role is bit-identical to the all-present launch (a workgroup that took
    another role's arguments, or another role's block index, shows here), an absent role's NaN-filled output stays NaN."""
    n = 33
    made = [_cell(I, H, 11 + r) for r, (I, H) in enumerate(ROLES)]
    cells = [c for _, c in made]
    xs, hs, reset = _inputs(ROLES, n, 7)
    full = _shared(cells, xs, hs, reset, n, {0, 1, 2, 3})
    assert all(bool(torch.isfinite(o).all()) for _, o in full)
    assert not torch.equal(full[0][1], full[2][1])                  # (the two 64-unit roles differ: a swapped pair would show)
    for mask in range(1, 16):
        present = {r for r in range(4) if mask >> r & 1}
        outs = _shared(cells, xs, hs, reset, n, present)
        for r in range(4):
            whole, got = outs[r]
            if r in present:
                assert torch.equal(got, full[r][1]), (mask, r)
                assert torch.isnan(whole[n:]).all(), (mask, r)
            else:
                assert torch.isnan(whole).all(), (mask, r)


def test_largest_staged_block_next_to_the_smallest_role():
    """(256, 256): the 67 584 B block above the default LDS limit and eight waves.  (1, 32): one wave, seven surplus waves that only meet
    the barrier, K = 33 with its pad row.  The small role sits in front of the large one and behind it."""
    for slots in ((1, 2), (3, 0)):
        _check_roles(((256, 256), (1, 32)), 33, 5, f"slots {slots}", slots=list(slots))


def test_error_codes_come_before_any_launch():
    from legged_games_gym_amd import capi
    lib = capi.load_dec_game_gru_library()
    err = lib.lg_dec_game_gru_last_error
    n = 33
    cells = [_cell(I, H, 11 + r)[1] for r, (I, H) in enumerate(ROLES)]
    xs, hs, reset = _inputs(ROLES, n, 3)
    outs = [_padded(n, H) for _, H in ROLES]

    def call(edit=None, num_envs=n, present=(0, 1, 2, 3)):
        roles = [[cells[r].handle, xs[r].data_ptr(), hs[r].data_ptr(), outs[r][1].data_ptr()] if r in present else None for r in range(4)]
        if edit:
            edit(roles)
        rc = lib.lg_dec_gru_step(capi.dec_gru_roles(roles), reset.data_ptr(), num_envs, _stream())
        return rc, err()

    assert lib.lg_dec_gru_step(None, reset.data_ptr(), n, _stream()) == -1 and b"null roles" in err()
    rc, text = call(present=())
    assert rc == -1 and b"all four handles are null" in text
    for r in range(4):
        for field in (1, 2, 3):                                     # x, h_in, h_out of a present role
            rc, text = call(lambda roles: roles[r].__setitem__(field, None))
            assert rc == -1 and b"null buffer" in text and NAMES[r].split("_")[1].encode() in text, (r, field, text)
        rc, text = call(lambda roles: roles[r].__setitem__(3, roles[r][2]))
        assert rc == -2 and b"alias" in text, (r, text)
    for bad in (0, -4):
        rc, text = call(num_envs=bad)
        assert rc == -2 and b"num_envs" in text

    class _Gru(ctypes.Structure):                                   # struct lg_gru in host memory, on another device: refused before the launch
        _fields_ = capi.lg_gru_handle._fields_
    elsewhere = _Gru(16, 64, 40, 1, None, None)
    rc, text = call(lambda roles: roles[2].__setitem__(0, ctypes.addressof(elsewhere)))
    assert rc == -2 and b"different devices" in text
    with pytest.raises(RuntimeError, match=r"lg_dec_gru_step failed \(-2\).*num_envs"):
        capi.dec_gru_step([None, None, (cells[2].handle, xs[2].data_ptr(), hs[2].data_ptr(), outs[2][1].data_ptr()), None], None, 0, _stream())
    with pytest.raises(ValueError, match="four roles"):
        capi.dec_gru_step([None] * 3, None, n, _stream())
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(whole).all()) for whole, _ in outs)  # nothing was launched
    rc, text = call()                                               # the same arguments unedited: accepted
    torch.cuda.synchronize()
    assert rc == 0 and all(bool(torch.isfinite(o).all()) for _, o in outs)


# ---------------------------------------------------------------------------------------------------------------- DecHighLevelGame
from tests.dec_game_fixtures import dec_registered  # noqa: E402,F401
from tests.test_gpu_dec_game import assert_same_state, make_dec  # noqa: E402
from tests.test_gpu_dec_game_recurrent import BIAS_PRED, BIAS_PREY, STD_PRED, STD_PREY  # noqa: E402
from tests.test_gpu_game import write_ll_checkpoint  # noqa: E402

N_GAME = 33
SEPARATE = "lg_lstm_actor_act x 2 + lg_dec_game_pre + lg_policy_act"


def _gru_policy(agent, units=64, hidden=(64, 64, 32), seed=6):
    from legged_games_gym_amd.rl import ActorCriticRecurrent
    no, na, bias, std = (16, 4, BIAS_PREY, STD_PREY) if agent == "prey" else (3, 2, BIAS_PRED, STD_PRED)
    torch.manual_seed(seed + no)
    ac = ActorCriticRecurrent(no, no, na, actor_hidden_dims=list(hidden), critic_hidden_dims=list(hidden), rnn_type="gru", rnn_hidden_size=units).to(DEV)
    with torch.no_grad():
        ac.std.copy_(torch.tensor(std))
        ac.actor[-1].bias.copy_(torch.tensor(bias))
    return ac


def _policies():
    if "policies" not in _cache:
        _cache["policies"] = (_gru_policy("pred"), _gru_policy("prey"))
    return _cache["policies"]


def _pair(shared, env=None, seeds=(21 + 104729, 21)):
    """Two ``RecurrentFusedActor(gru=True)`` over the same two GRU modules; on ``env``'s device step counter when given."""
    from legged_games_gym_amd.rl.recurrent_actor import RecurrentFusedActor
    ctr = None if env is None else env.ll_env._sim.buf["step_counter"]
    return tuple(RecurrentFusedActor(ac, DEV, seed=s, step_counter=ctr, num_envs=N_GAME, gru=True, shared_gru=shared) for ac, s in zip(_policies(), seeds))


def _two_envs(tmp_path, seed=9, reset_seed=90):
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)         # a random low-level policy
    A, B = make_dec(ckpt, N_GAME, seed=seed), make_dec(ckpt, N_GAME, seed=seed)
    for env in (A, B):
        torch.manual_seed(reset_seed)                                              # reset_idx from the host draws from torch's generator
        env.reset()
        env.ll_env.episode_length_buf[::2] = int(env.ll_env.max_episode_length) - 2 - (torch.arange(0, N_GAME, 2, device=DEV) % 7)
    assert torch.equal(A.obs_buf_prey, B.obs_buf_prey) and torch.equal(A.ll_env.root_states, B.ll_env.root_states)
    return A, B


def _same_memories(fa, fb):
    return all(len(pa) == 1 and torch.equal(pa[0], pb[0]) for pa, pb in zip(fa.hidden_states(), fb.hidden_states()))


def _outputs(sample=True):
    """Per agent the optional outputs a rollout asks for; without ``sample`` the env keeps the sample the log-prob is taken of itself."""
    return tuple(dict(log_prob=torch.empty(N_GAME, device=DEV), **({"sample": torch.empty(N_GAME, w, device=DEV)} if sample else {})) for w in (2, 4))


def _counted(monkeypatch):
    """Count the calls of ``capi.dec_gru_step`` and ``capi.dec_game_lstm_act`` (the return codes of the latter)."""
    from legged_games_gym_amd import capi
    cell, act, real_cell, real_act = [], [], capi.dec_gru_step, capi.dec_game_lstm_act
    monkeypatch.setattr(capi, "dec_gru_step", lambda *a, **k: cell.append(1) or real_cell(*a, **k))
    monkeypatch.setattr(capi, "dec_game_lstm_act", lambda *a, **k: act.append(real_act(*a, **k)) or act[-1])
    return cell, act


def _step_both(A, B, actors_a, actors_b, k, capsys, critics=("pred",)):
    """One ``step_policy`` on each env with every optional output compared bit for bit (the log-probs too: with the shared launches the env
    fills them in from torch as the separate launches do); returns what each env printed."""
    (pa, ya), (pb, yb) = actors_a, actors_b
    (op_a, oy_a), (op_b, oy_b) = _outputs(k % 2 == 0), _outputs(k % 2 == 0)      # every other step: the log-prob without the sample
    capsys.readouterr()
    pred_a, prey_a, res_a = A.step_policy(pa, ya, out_pred=op_a, out_prey=oy_a, with_critic_memory=critics)
    said_a = capsys.readouterr().out
    pred_b, prey_b, res_b = B.step_policy(pb, yb, out_pred=op_b, out_prey=oy_b, with_critic_memory=critics)
    said_b = capsys.readouterr().out
    torch.cuda.synchronize()
    assert len(pred_a) == len(pred_b) == (3 if "pred" in critics else 2) and len(prey_a) == len(prey_b) == 2, k
    for x, y in zip(pred_a + prey_a, pred_b + prey_b):              # commands, means, the learner's critic memory
        assert bool(torch.isfinite(x).all()) and torch.equal(x, y), k
    for da, db in ((op_a, op_b), (oy_a, oy_b)):
        for key in da:                                              # samples and log-probs
            assert bool(torch.isfinite(da[key]).all()) and torch.equal(da[key], db[key]), (k, key)
    for x, y in zip(res_a, res_b):                                  # observations, rewards, dones
        if torch.is_tensor(x):
            assert torch.equal(x, y), k
    assert_same_state(A, B, k)
    assert _same_memories(pa, pb) and _same_memories(ya, yb), k
    assert pa._flip == pb._flip and ya._flip == yb._flip, k
    return said_a, said_b


def test_two_envs_side_by_side_shared_against_separate_launches(tmp_path, monkeypatch, capsys):
    """A: two GRU actors with ``shared_gru`` (``lg_dec_gru_step`` -> ``lg_dec_game_lstm_act``).  B, identically seeded: the same modules
    without it (``lg_gru_step`` x 2, ``lg_lstm_actor_act`` x 2, ``lg_dec_game_pre``, ``lg_policy_act``).  Four policy steps, a reset forced in
    between, the predator's critic memory in the launch."""
    A, B = _two_envs(tmp_path)
    actors_a, actors_b = _pair(True), _pair(False)
    assert all(f.gru and f.shared_gru for f in actors_a) and all(f.gru and not f.shared_gru for f in actors_b)
    cell, act = _counted(monkeypatch)
    forced = torch.arange(3, N_GAME, 5, device=DEV)
    said_a, said_b, resets = "", "", 0
    for k in range(4):
        a, b = _step_both(A, B, actors_a, actors_b, k, capsys)
        said_a, said_b = said_a + a, said_b + b
        assert A.last_act_rc == 0 and B.last_act_rc == -4, k
        resets += int(A.reset_buf.sum())
        for env in (A, B):
            env.reset_buf[forced] = True
    assert len(cell) == 4 and act == [0] * 4                         # A's two launches per step; B reached neither
    assert resets > 0 and all(float(f.hidden_states()[0][0].abs().max()) > 0.0 for f in actors_a)
    assert float(actors_a[0].hidden_states()[1][0].abs().max()) > 0.0 and float(actors_a[1].hidden_states()[1][0].abs().max()) == 0.0
    assert "unavailable" not in said_a, said_a
    lines = [l for l in said_b.splitlines() if "unavailable" in l]
    assert len(lines) == 1 and "GRU memory" in lines[0] and SEPARATE in lines[0], said_b
    # a mixed pair stays where it is today: separate launches, the same line
    mixed = (_pair(True)[0], _pair(False)[1])
    assert A._recurrent_launches(*mixed, say=False) == (None, False) and A.shared_actor_launch(*mixed) is False


@pytest.mark.parametrize("steps_per_replay", [1, 2])
def test_graphed_policy_step_equals_the_eager_separate_launches(tmp_path, monkeypatch, capsys, steps_per_replay):
    """Memories from zero on the sims' device step counters: the warm-up call, three warm-up steps and the capture on A (shared launches),
    the same steps eagerly on B (separate launches); four replays.  Then, at wide precision 0, A's actors take the separate launches
    (rc -4, the existing message) while its memories still move in the shared cell launch."""
    from legged_games_gym_amd import capi
    A, B = _two_envs(tmp_path)
    (pa, ya), (pb, yb) = _pair(True, A), _pair(False, B)
    capsys.readouterr()
    assert A.shared_actor_launch(pa, ya) is True and B.shared_actor_launch(pb, yb) is False
    assert not any(float(t.abs().max()) for f in (pa, ya) for st in f.hidden_states() for t in st)      # the warm-up moved no memory
    replay = A.make_graphed_policy_step(pa, ya, warmup=3, steps_per_replay=steps_per_replay)
    assert A.last_act_rc == 0 and "unavailable" not in capsys.readouterr().out
    for _ in range(3):
        B.step_policy(pb, yb)
    for k in range(4):
        replay()
        for _ in range(steps_per_replay):
            B.step_policy(pb, yb)
        torch.cuda.synchronize()
        for fa, fb in ((pa, pb), (ya, yb)):
            assert all(torch.equal(a, b) for a, b in zip(fa.output_buffers(N_GAME), fb.output_buffers(N_GAME))), k
            assert torch.equal(fa.hidden_states()[0][0], fb.hidden_states()[0][0]), k      # the actor memories
        assert_same_state(A, B, k)
        assert int(A.ll_env._sim.buf["step_counter"][0]) == A.ll_env.common_step_counter == B.ll_env.common_step_counter
    assert float(pa.hidden_states()[0][0].abs().max()) > 0.0 and float(ya.hidden_states()[0][0].abs().max()) > 0.0

    lib = capi.load_library()
    cell, act = _counted(monkeypatch)
    actors_a, actors_b = _pair(True), _pair(False)                   # host-counted noise streams, memories from zero on both
    old = lib.lg_mlp_wide_set_precision(0)
    try:
        said = ""
        for k in range(2):
            a, _ = _step_both(A, B, actors_a, actors_b, 10 + k, capsys)
            said += a
            assert A.last_act_rc == -4, k
        assert len(cell) == 2 and act == []                          # the cell launch stayed shared, the actor launch was not tried
        assert said.count("\n") == 1 and "wide precision 0" in said and SEPARATE in said, said
        assert A.shared_actor_launch(*actors_a) is False
    finally:
        lib.lg_mlp_wide_set_precision(old)
    assert lib.lg_mlp_wide_set_precision(-1) == 1


def test_env_takes_the_separate_launches_without_the_library(tmp_path, monkeypatch, capsys):
    """Without liblegged_dec_game_gru.so everything is separate launches, with one line that names the library; the results are the same."""
    from legged_games_gym_amd import capi
    A, B = _two_envs(tmp_path)
    actors_a, actors_b = _pair(True), _pair(False)
    monkeypatch.setattr(capi.LIBRARIES["dec_game_gru"], "handle", None)
    monkeypatch.setenv("LG_DEC_GAME_GRU_LIB", str(tmp_path / "liblegged_dec_game_gru_absent.so"))
    cell, act = _counted(monkeypatch)
    said = ""
    for k in range(2):
        said += _step_both(A, B, actors_a, actors_b, k, capsys)[0]
        assert A.last_act_rc == -4
    assert cell == [] and act == []
    assert said.count("\n") == 1 and "liblegged_dec_game_gru_absent.so" in said and SEPARATE in said, said
    assert A.shared_actor_launch(*actors_a) is False


# ---------------------------------------------------------------------------------------------------------------- DecGamePolicyRunner
RUNNER_KEYS = ("device_rollout", "policy_class_name", "device_gru", "dec_gru_shared")


def _dec_runner(reg, root, monkeypatch, ckpt, n=N_GAME, units=64, **runner_keys):
    """``dec_high_level_game`` with two GRU policies of ``units`` units on the device rollout and the runner keys given; time-outs of the
    low-level env inside the first rollouts."""
    import legged_games_gym_amd.utils.task_registry as tr_mod
    from legged_games_gym_amd.utils import get_args
    from legged_games_gym_amd.utils.helpers import apply_policy_args
    monkeypatch.setattr(tr_mod, "LEGGED_GYM_ROOT_DIR", str(root))
    env_cfg, train_cfg = reg.get_cfgs("dec_high_level_game")
    env_cfg.env.ll_policy_path = ckpt
    if hasattr(train_cfg.runner, "graphed_rollout"):
        delattr(train_cfg.runner, "graphed_rollout")
    train_cfg.runner.device_rollout = True                                  # runner keys, not config fields: set on this registration only
    for key, value in runner_keys.items():
        setattr(train_cfg.runner, key, value)
    args = get_args(["--task", "dec_high_level_game", "--num_envs", str(n), "--headless", "--sim_device", DEV, "--rl_device", DEV,
                     "--policy_class_name", "ActorCriticRecurrent", "--rnn_type", "gru", "--rnn_hidden_size", str(units)])
    apply_policy_args(train_cfg, args)
    env, _ = reg.make_env("dec_high_level_game", args)
    torch.manual_seed(1234)
    runner, _ = reg.make_dec_alg_runner(env, "dec_high_level_game", args)
    env.ll_env.episode_length_buf[::2] = int(env.ll_env.max_episode_length) - 3 - (torch.arange(0, n, 2, device=DEV) % 41)
    return env, runner, args


def _restore(reg):
    _, train_cfg = reg.get_cfgs("dec_high_level_game")               # the registered object is shared: leave it as it was found
    for obj, keys in ((train_cfg.runner, RUNNER_KEYS), (train_cfg.policy, ("rnn_hidden_size", "rnn_type"))):
        for key in keys:
            if key in vars(obj):
                delattr(obj, key)


def test_dec_runner_trains_two_gru_policies_on_the_shared_launches(tmp_path, monkeypatch, dec_registered, capsys):
    from legged_games_gym_amd.rl.recurrent_actor import RecurrentFusedActor
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    try:
        env, runner, _ = _dec_runner(dec_registered, tmp_path / "run", monkeypatch, ckpt, device_gru=True, dec_gru_shared=True)
        assert runner.recurrent and runner.device_path and env.num_envs == N_GAME
        fused = {a: runner.runners[a]._fused for a in ("pred", "prey")}
        for a in ("pred", "prey"):
            r = runner.runners[a]
            assert isinstance(fused[a], RecurrentFusedActor) and fused[a].gru and fused[a].shared_gru and r._game_rollout and r._recurrent_rollout
            assert isinstance(r.alg.actor_critic.memory_a.rnn, nn.GRU) and r.alg.actor_critic.memory_a.rnn.hidden_size == 64
        assert env.shared_actor_launch(fused["pred"], fused["prey"]) is True
        cell, act = _counted(monkeypatch)
        losses = {}
        for a in ("pred", "prey"):
            alg = runner.runners[a].alg

            def update(_update=alg.update, _a=a):
                losses.setdefault(_a, []).append(_update())
                return losses[_a][-1]
            monkeypatch.setattr(alg, "update", update)
        params = lambda a: [p.detach().clone() for p in runner.runners[a].alg.actor_critic.parameters()]
        before = {a: params(a) for a in ("pred", "prey")}
        runner.learn(max_num_evolutions=1, num_learning_iterations=2)            # the predator learns; the prey's actor memory moves as its opponent
        torch.cuda.synchronize()
        carried = fused["prey"].hidden_states()[0][0].clone()
        assert float(carried.abs().max()) > 0.0 and set(losses) == {"pred"}
        seen = {}
        r = runner.runners["prey"]

        def learn(*x, _learn=r.learn, **k):                                       # what the prey's evolution starts from
            seen["actor"] = fused["prey"].hidden_states()[0][0].clone()
            return _learn(*x, **k)
        r.learn = learn
        runner.learn(max_num_evolutions=1, num_learning_iterations=2)
        torch.cuda.synchronize()
        assert torch.equal(seen["actor"], carried)                                # the opponent's actor memory carried across the evolutions
        assert runner.current_evolution == 2 and {a: len(v) for a, v in losses.items()} == {"pred": 2, "prey": 2}
        assert all(np.isfinite(v) for per in losses.values() for pair in per for v in pair), losses
        assert all(bool(torch.isfinite(p).all()) for a in ("pred", "prey") for p in runner.runners[a].alg.actor_critic.parameters())
        assert all(any(not torch.equal(x, y) for x, y in zip(before[a], params(a))) for a in ("pred", "prey"))
        assert len(cell) > 0 and len(cell) == len(act) and set(act) == {0}        # every policy step: the two shared launches
        assert "unavailable" not in capsys.readouterr().out
    finally:
        _restore(dec_registered)


def test_dec_runner_without_the_key_takes_the_separate_launches_and_says_so(tmp_path, monkeypatch, dec_registered, capsys):
    """The default next to the opt-in: ``device_gru`` alone keeps the six launches and the one "GRU memory" line."""
    ckpt = write_ll_checkpoint(str(tmp_path / "ll" / "model_0.pt"), seed=3)
    try:
        env, runner, _ = _dec_runner(dec_registered, tmp_path / "run", monkeypatch, ckpt, device_gru=True)
        fused = {a: runner.runners[a]._fused for a in ("pred", "prey")}
        assert all(f.gru and not f.shared_gru for f in fused.values())
        assert env.shared_actor_launch(fused["pred"], fused["prey"]) is False
        cell, act = _counted(monkeypatch)
        runner.learn(max_num_evolutions=1, num_learning_iterations=1)
        torch.cuda.synchronize()
        assert cell == [] and act == []
        said = capsys.readouterr().out
        lines = [l for l in said.splitlines() if "unavailable" in l]
        assert len(lines) == 1 and "GRU memory" in lines[0] and SEPARATE in lines[0], said
    finally:
        _restore(dec_registered)
