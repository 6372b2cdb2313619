"""The restatements of tests/ppo_tail_ref.py, checked without a GPU: in float64 against the project's torch paths (1e-12 relative), the
tolerance rule and the guard bands on what they must refuse, the input conditions of every case tests/test_gpu_ppo_tail.py runs, and --
through the restatements at float32 -- that the bound separates a correct kernel from the arithmetic slips it is there to catch."""
import math

import pytest
import torch

from tests import ppo_tail_ref as R

F32, F64 = torch.float32, torch.float64
REL = 1e-12


def close(a, b, rel=REL):
    a, b = a.double(), b.double()
    return R.err(a, b) <= rel * max(1.0, float(b.abs().max()) if b.numel() else 0.0)


# ------------------------------------------------------------------------------------------------ restatements against the torch paths
class _DoublesForFloat:
    """``dones`` for RolloutStorage._gae_torch on double tensors: the scan asks for ``dones[step].float()``, and a float32 ``not_done``
    times the Python float ``gamma`` would round gamma to float32 (1e-8, far above the 1e-12 asked here).  ``.float()`` answers in float64.
    Not a tensor on purpose: it has ``[step]`` and ``.float()`` and nothing else, so a scan that reads the flags any other way (``.to()``,
    ``.bool()``, arithmetic on ``dones[step]``) fails here with an AttributeError / TypeError instead of passing in float32; the scan says so."""

    def __init__(self, dones):
        self.dones = dones

    def __getitem__(self, step):
        return _DoublesForFloat(self.dones[step])

    def float(self):
        return self.dones.double()


@pytest.mark.parametrize("case", R.GAE_CASES, ids=R.GAE_IDS)
def test_gae_restatement_equals_the_storage_scan_in_float64(case):
    from legged_games_gym_amd.rl.ppo import RolloutStorage
    inp = R.gae_inputs(case)
    st = RolloutStorage.__new__(RolloutStorage)
    st.num_transitions_per_env = inp["T"]
    st.rewards, st.values = inp["rewards"].double().unsqueeze(-1), inp["values"].double().unsqueeze(-1)
    st.dones = _DoublesForFloat(inp["dones"].unsqueeze(-1))
    st.returns, st.advantages = torch.zeros_like(st.rewards), torch.zeros_like(st.rewards)
    st._gae_torch(inp["last_values"].double().unsqueeze(-1), inp["gamma"], inp["lam"])
    ret, adv = R.gae(inp["rewards"], inp["values"], inp["dones"], inp["last_values"], inp["gamma"], inp["lam"], F64)
    assert bool(torch.isfinite(ret).all()) and close(ret, st.returns[..., 0]) and close(adv, st.advantages[..., 0])
    # an env that is done at T - 1 returns its own reward there, whatever last_values holds
    e = int(torch.nonzero(inp["dones"][-1])[0])
    assert inp["last_values"][e] == R.HUGE
    assert abs(float(ret[-1, e]) - float(inp["rewards"][-1, e])) <= 1e-15 * max(1.0, abs(float(inp["values"][-1, e])))


@pytest.mark.parametrize("kl_cycle", [("above", "below", "equal"), ("above_clamped", "below_clamped", "zero"), ("on_upper", "on_lower", "null", "desired_zero")])
def test_adam_restatement_equals_clip_grad_norm_and_torch_adam_in_float64(kl_cycle):
    """Seven steps on double tensors: the reference order (KL rule on the learning rate, clip_grad_norm_, optimizer.step()), the KL mode
    cycling through ``kl_cycle`` with the learning rate each mode starts from, gradients alternating around max_norm."""
    shapes = R.ADAM_LISTS["small_beside_large"][:5] + [(64, 48)]
    g = torch.Generator().manual_seed(5)
    params = [torch.nn.Parameter(torch.randn(s, generator=g, dtype=F64) * 1e-2) for s in shapes]
    opt = torch.optim.Adam(params, lr=1e-3, betas=R.BETAS, eps=R.EPS)
    mine = dict(p=[p.detach().clone() for p in params], m=[torch.zeros(s, dtype=F64) for s in shapes], v=[torch.zeros(s, dtype=F64) for s in shapes],
                steps=[0.0] * len(shapes))
    for it in range(7):
        kl, lr0, desired, _ = R.KL_MODES[kl_cycle[it % len(kl_cycle)]]
        kl = None if kl is None else R.f32(kl)
        grads = [torch.randn(s, generator=g, dtype=F64) * (3.0 if it % 2 else 0.01) for s in shapes]
        lr = lr0
        if kl is not None and desired > 0:                       # rsl_rl PPO.update
            if kl > R.D32 * 2.0:
                lr = max(1e-5, lr / 1.5)
            elif kl < R.D32 / 2.0 and kl > 0.0:
                lr = min(1e-2, lr * 1.5)
        for group in opt.param_groups:
            group["lr"] = lr
        for p, x in zip(params, grads):
            p.grad = x.clone()
        norm = torch.nn.utils.clip_grad_norm_(params, R.MAX_NORM)
        opt.step()
        mine["p"], mine["m"], mine["v"], mine["steps"], got_lr, got_norm, coef = R.adam_step(mine["p"], grads, mine["m"], mine["v"], mine["steps"], lr0, R.BETAS, R.EPS,
                                                                                             R.MAX_NORM, kl, desired, F64)
        assert abs(float(got_lr) - lr) <= REL * lr and abs(float(got_norm) - float(norm)) <= REL * float(norm)
        assert (float(coef) == 1.0) == (float(norm) + 1e-6 <= R.MAX_NORM)
        for k, p in enumerate(params):
            s = opt.state[p]
            assert close(mine["p"][k], p.detach()) and close(mine["m"][k], s["exp_avg"]) and close(mine["v"][k], s["exp_avg_sq"]), (it, k)
            assert float(s["step"]) == mine["steps"][k] == it + 1
    assert {R.KL_MODES[k][0] for k in kl_cycle} != {None}


def test_kl_rule_of_the_restatement_on_every_mode():
    for name, (kl, lr0, desired, after) in R.KL_MODES.items():
        for dtype in (F32, F64):
            lr = R.adam_step([torch.zeros(1)], [torch.zeros(1)], [torch.zeros(1)], [torch.ones(1)], [0.0], R.f32(lr0), R.BETAS, R.EPS, R.MAX_NORM,
                             None if kl is None else R.f32(kl), desired, dtype)[4]
            assert lr.dtype == dtype and abs(float(lr) - after(lr0)) <= 2e-7 * after(lr0), (name, dtype, float(lr))
            if name in ("equal", "zero", "on_upper", "on_lower", "null", "desired_zero"):
                assert float(lr) == R.f32(lr0), name                                    # unchanged means untouched


@pytest.mark.parametrize("A", [2, 3, 4, 6, 12, 16])
def test_log_prob_restatement_equals_torch_normal_in_float64(A):
    g = torch.Generator().manual_seed(A)
    std = R.policy_std(A, g).double()
    mean = torch.randn(200, A, generator=g, dtype=F64)
    act = mean + std * torch.randn(200, A, generator=g, dtype=F64)
    want = torch.distributions.Normal(mean, std.expand_as(mean)).log_prob(act).sum(-1)
    assert close(R.log_prob(act, mean, std, F64), want)


@pytest.mark.parametrize("case", R.RECORD_CASES, ids=str)
def test_episode_statistics_equal_the_tensor_op_version_in_float64(case):
    """record step by step and finish over the same steps against the tensor-op bookkeeping of
    tests/test_gpu_rl.py::test_rollout_record_kernel_matches_the_torch_bookkeeping."""
    N, O, A = case
    inp = R.record_inputs(case)
    ref = {"cur_rew": inp["cur_return"].double(), "cur_len": inp["cur_length"].double(), "sums": inp["sums"].double()}
    cr, cl, sums = inp["cur_return"], inp["cur_length"], inp["sums"]
    for t in range(R.RECORD_STEPS):
        out = R.record(inp["obs"][t], inp["actions"][t], inp["mean"][t], inp["rewards"][t], inp["dones"][t], inp["time_outs"][t], inp["std"], cr, cl, sums, F64)
        cr, cl, sums = out["cur_return"], out["cur_length"], out["sums"]
        d = inp["dones"][t].double()
        ref["cur_rew"] = ref["cur_rew"] + inp["rewards"][t].double(); ref["cur_len"] = ref["cur_len"] + 1.0
        ref["sums"] = ref["sums"] + torch.stack(((ref["cur_rew"] * d).sum(), (ref["cur_len"] * d).sum(), d.sum()))
        ref["cur_rew"] = ref["cur_rew"] * (1.0 - d); ref["cur_len"] = ref["cur_len"] * (1.0 - d)
        assert torch.equal(out["time_outs"], inp["time_outs"][t].float()) and torch.equal(out["sigma"], inp["std"].expand(N, A))
        assert torch.equal(out["obs"], inp["obs"][t]) and torch.equal(out["dones"], inp["dones"][t])
    assert close(cr, ref["cur_rew"]) and torch.equal(cl, ref["cur_len"]) and close(sums, ref["sums"])
    seg = R.finish(inp["actions"], inp["mean"], inp["rewards"], inp["dones"], inp["time_outs"], inp["std"], inp["cur_return"], inp["cur_length"], inp["sums"], F64)
    assert close(seg["cur_return"], cr) and torch.equal(seg["cur_length"], cl) and close(seg["sums"], sums)
    assert seg["terms"].numel() == int(inp["dones"].sum()) == int(sums[2] - R.SUMS0[2])
    assert seg["log_prob"].shape == (R.RECORD_STEPS, N) and torch.equal(seg["time_outs"], inp["time_outs"].float())
    # without the optional inputs
    bare = R.record(inp["obs"][0], inp["actions"][0], inp["mean"][0], inp["rewards"][0], inp["dones"][0], None, None, None, None, None, F64)
    assert "sigma" not in bare and "log_prob" not in bare and "sums" not in bare and not bool(bare["time_outs"].any())


# ------------------------------------------------------------------------------------------------ the rule and the bands refuse what they must
def test_bound_and_check_catch_a_perturbed_copy():
    g = torch.Generator().manual_seed(0)
    want = torch.randn(1000, generator=g, dtype=F64) * 40.0
    want32 = want.float()
    e32 = R.err(want32, want)
    assert R.bound(e32, want) == 4.0 * max(e32, R.ULP * float(want.abs().max()))
    assert R.bound(0.0, want) == 4.0 * R.ULP * float(want.abs().max()) > 0.0             # the floor
    assert R.bound(1.0, want, margin=2.0) == 2.0
    lines = []
    assert R.check("copy", want32.clone(), want, want32, out=lines.append) == 1.0
    assert len(lines) == 1 and lines[0].startswith("[observed] copy: kernel ")
    bad = want32.clone()
    bad[137] += 1.01 * R.bound(e32, want)
    with pytest.raises(AssertionError, match="max error"):
        R.check("perturbed", bad, want, want32, out=lines.append)
    nan = want32.clone()
    nan[3] = float("nan")
    with pytest.raises(AssertionError, match="non-finite"):
        R.check("nan", nan, want, want32, out=lines.append)
    with pytest.raises(AssertionError, match="shapes"):
        R.check("shape", want32[:-1], want, want32, out=lines.append)
    ok = want32.clone()
    ok[137] += 0.5 * R.bound(e32, want)
    R.check("inside", ok, want, want32, out=lines.append)


def test_sum_bound_holds_for_every_order_and_is_not_slack():
    g = torch.Generator().manual_seed(1)
    x32 = torch.cat((torch.tensor([5.5]), torch.randn(300, generator=g) * 7.0))
    exact = float(x32.double().sum())
    worst = 0.0
    for k in range(20):
        order = torch.randperm(301, generator=g)
        s = torch.zeros((), dtype=F32)
        for v in x32[order]:
            s = s + v
        b = R.sum_bound(x32, float(s))
        worst = max(worst, abs(float(s) - exact) / b)
        assert abs(float(s) - exact) <= b
    assert worst > 1e-3                                                                 # within three orders of magnitude of what is observed
    assert R.sum_bound(x32, exact) < 1e-3 * abs(exact) and abs(exact) * 0.001 > R.sum_bound(x32, exact)          # a sum off by 0.1 % is caught
    assert R.sum_bound(x32[:1], 5.5) == 2.0 ** -21                                      # one term: the spacing at the result alone


@pytest.mark.parametrize("dtype", [F32, torch.uint8])
def test_guard_bands_catch_a_touched_band(dtype):
    G = R.Guarded((5, 7), dtype)
    assert G.t.shape == (5, 7) and G.untouched() and G.buf.numel() == 35 + 2 * R.GUARD and G.ptr() == G.buf.data_ptr() + R.GUARD * G.buf.element_size()
    G.t.fill_(1)
    G.check("filled")
    assert not G.untouched()
    for where in (R.GUARD - 1, R.GUARD + 35, 0, G.buf.numel() - 1):
        H = R.Guarded((5, 7), dtype)
        H.buf[where] = 1
        with pytest.raises(AssertionError, match="band"):
            H.check("touched")
    init = R.Guarded(3, F32, init=torch.tensor([1.0, 2.0, 3.0]))
    assert init.t.tolist() == [1.0, 2.0, 3.0]
    init.check()


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests
@pytest.mark.parametrize("case", R.GAE_CASES, ids=R.GAE_IDS)
def test_gae_cases_hold_their_input_conditions(case):
    R.assert_gae_inputs(R.gae_inputs(case))


def test_gae_cases_are_the_listed_shapes():
    assert [(c[1], c[2]) for c in R.GAE_CASES] == [(1, 1), (1, 257), (24, 255), (24, 256), (24, 777), (100, 300), (64, 257)]
    assert R.GAE_CASES[5][3:5] == (0.999, 0.99) and R.GAE_CASES[6][5:] == (30.0, 1.0)


@pytest.mark.parametrize("case", R.ADAM_CASES, ids=R.ADAM_IDS)
def test_adam_cases_hold_their_input_conditions(case):
    inp = R.adam_inputs(case)
    R.assert_adam_inputs(inp)
    p, m, v, steps, lr, norm, coef = R.adam_restated(inp, F64)
    assert abs(float(lr) - inp["lr_after"](inp["lr"])) <= 1e-7 * float(lr)
    assert (float(coef) == 1.0) == (inp["grad_mode"] != "above") and all(bool(torch.isfinite(x).all()) for x in p + m + v)
    moved = max(R.err(a, b) for a, b in zip(p, inp["params"]))
    assert 1e-6 < moved < 0.1, moved                                  # the update is far above the rounding of a stored parameter (6e-10)


def test_adam_cases_cover_every_list_step_count_gradient_mode_and_kl_mode():
    lists, steps, grads, kls = (set(c[i] for c in R.ADAM_CASES) for i in range(4))
    assert lists == set(R.ADAM_LISTS) - {"thirty_three"} and steps == set(R.STEP_COUNTS) and grads == set(R.GRAD_NORMS) and kls == set(R.KL_MODES)
    big = R.ADAM_LISTS["small_beside_large"]
    assert [math.prod(s) for s in big] == [1, 3, 255, 256, 257, 120320]
    chunk = (120320 + 63) // 64
    assert all(math.prod(s) % chunk for s in big[:-1]) and 120320 % chunk == 0 and 3 // chunk == 0          # 63 empty chunks beside the large tensor
    assert len(R.ADAM_LISTS["thirty_three"]) == 33


@pytest.mark.parametrize("case", R.RECORD_CASES, ids=str)
def test_record_cases_hold_their_input_conditions(case):
    R.assert_record_inputs(case, R.record_inputs(case))
    assert case[2] <= case[1] and case[2] <= 16


@pytest.mark.parametrize("case", R.FINISH_CASES, ids=str)
def test_finish_cases_hold_their_input_conditions(case):
    R.assert_finish_inputs(case, R.finish_inputs(case))


def test_case_lists_are_the_listed_shapes():
    assert R.RECORD_CASES == [(1, 3, 2), (17, 3, 3), (33, 16, 4), (257, 19, 6), (130, 235, 12), (50, 20, 16)]
    assert R.FINISH_CASES == [(1, 1, 2), (3, 5, 3), (24, 33, 12), (7, 257, 16), (24, 200, 12)]
    assert any(n == o for _, o, n in R.RECORD_CASES)


# ------------------------------------------------------------------------------------------------ the bound bites
def _caught(got32, want, want32):
    return R.err(got32, want) >= R.bound(R.err(want32, want), want)


@pytest.mark.parametrize("case", R.GAE_CASES[2:], ids=R.GAE_IDS[2:])
def test_bound_separates_gae_slips(case):
    """gamma * lam -> gamma in the recursion misses the bound; advantages stored as the running advantage instead of
    (advantage + value) - value are within it but not bit-equal to returns - values."""
    inp = R.gae_inputs(case)
    a = (inp["rewards"], inp["values"], inp["dones"], inp["last_values"], inp["gamma"])
    want, _ = R.gae(*a, inp["lam"], F64)
    want32, adv32 = R.gae(*a, inp["lam"], F32)
    assert _caught(R.gae(*a, 1.0, F32)[0], want, want32)
    assert torch.equal(adv32, want32 - inp["values"])
    running = torch.zeros_like(want32)
    adv = torch.zeros(inp["N"])
    for t in reversed(range(inp["T"])):
        nxt = inp["last_values"] if t == inp["T"] - 1 else inp["values"][t + 1]
        nd = 1.0 - inp["dones"][t].float()
        adv = inp["rewards"][t] + nd * inp["gamma"] * nxt - inp["values"][t] + nd * inp["gamma"] * inp["lam"] * adv
        running[t] = adv
    assert not torch.equal(running, adv32) and not _caught(running, want - inp["values"].double(), adv32)


@pytest.mark.parametrize("case", [c for c in R.ADAM_CASES if c[1] <= 999 and c[2] != "zero"], ids=[i for c, i in zip(R.ADAM_CASES, R.ADAM_IDS) if c[1] <= 999 and c[2] != "zero"])
def test_bound_separates_adam_slips(case):
    """An update off by 0.2 % (a few 1e-6 on the parameters) and a dropped sqrt(bias_correction2) both miss the bound on the parameters."""
    inp = R.adam_inputs(case)
    want, want32 = R.adam_restated(inp, F64), R.adam_restated(inp, F32)
    for k in range(len(want[0])):
        R.check(f"params[{k}]", want32[0][k], want[0][k], want32[0][k], out=lambda s: None)
    off = [p0 + (p1 - p0) * 1.002 for p0, p1 in zip(inp["params"], want32[0])]
    assert any(_caught(o, w, w32) for o, w, w32 in zip(off, want[0], want32[0]))
    bc2 = 1.0 - R.BETAS[1] ** (case[1] + 1)
    dropped = [p0 + (p1 - p0) / math.sqrt(bc2) for p0, p1 in zip(inp["params"], want32[0])]          # (eps is negligible beside sqrt(v))
    assert any(_caught(o, w, w32) for o, w, w32 in zip(dropped, want[0], want32[0]))


@pytest.mark.parametrize("case", R.FINISH_CASES, ids=str)
def test_bound_separates_a_shortened_log_prob_constant(case):
    """0.918938533 -> 0.91893 (8.5e-6 per action) misses the bound at every action count of the cases."""
    inp = R.finish_inputs(case)
    want, want32 = (R.log_prob(inp["actions"], inp["mean"], inp["std"], d) for d in (F64, F32))
    slipped = want32 + case[2] * (0.918938533 - 0.91893)
    assert _caught(slipped, want, want32), (R.err(slipped, want), R.bound(R.err(want32, want), want))
