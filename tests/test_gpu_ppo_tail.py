"""-m gpu: the tail of every PPO iteration -- ``lg_gae_returns`` (k_gae), ``lg_adam_step`` (k_adam_sumsq / k_adam_prepare /
k_adam_update), ``lg_rollout_record`` and ``lg_rollout_finish`` (k_rollout_record / k_rollout_post) -- against the float64 restatements of
tests/ppo_tail_ref.py, at the smallest shapes at which the kernels' branches differ.

Tolerance (tests/ppo_tail_ref.py: ``bound`` / ``check``): for every floating-point quantity, on the same inputs, ``want`` is the restatement
at float64 and ``e32`` the largest distance of the restatement at float32 from it; the kernel must be within 4 x max(e32, 2^-23 max |want|).
These kernels are built with 1-ulp divide / square root and use __logf, so nothing tighter than "as good as float32 torch" is claimed, and
nothing looser is accepted.  Quantities that involve no rounding (copies, flags, counts, lengths, step counters) are compared with
``torch.equal``.  Every buffer a kernel writes lies between guard bands (``Guarded``) and, where it holds no state, starts as NaN / 0xFF.
The figures are printed as ``[observed] ...``; the case lists and their seeded inputs are those of tests/ppo_tail_ref.py, whose input
conditions tests/test_ppo_tail_ref.py asserts without a GPU."""
import pytest
import torch

from tests import ppo_tail_ref as R
from tests.ppo_tail_ref import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64


def _lib():
    from legged_games_gym_amd import capi
    return capi.load_library()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _refused(L, rc):
    """An entry point refused its arguments: -1 and a message."""
    assert rc == -1, rc
    assert len(L.lg_last_error().decode()) > 0


def _flat(tensors):
    return torch.cat([t.detach().reshape(-1).cpu() for t in tensors])


# ------------------------------------------------------------------------------------------------ GAE
def _gae_device(inp):
    return {k: inp[k].to(DEV) for k in ("rewards", "values", "dones", "last_values")}


@pytest.mark.parametrize("case", R.GAE_CASES, ids=R.GAE_IDS)
def test_gae_kernel_matches_float64(case):
    """k_gae at one env, one step, a workgroup edge on either side (255 / 256 / 257), several workgroups, long memory and large values.
    Largest kernel / e32 on the MI355X: returns 1.03, advantages 1.02 (T = 100, gamma 0.999; 1.00 in the other cases)."""
    L = _lib()
    inp = R.gae_inputs(case)
    R.assert_gae_inputs(inp)
    T, N = inp["T"], inp["N"]
    d = _gae_device(inp)
    ret, adv = Guarded((T, N), device=DEV), Guarded((T, N), device=DEV)
    rc = L.lg_gae_returns(d["rewards"].data_ptr(), d["values"].data_ptr(), d["dones"].data_ptr(), d["last_values"].data_ptr(), inp["gamma"], inp["lam"],
                          ret.ptr(), adv.ptr(), T, N, _stream())
    assert rc == 0, L.lg_last_error()
    torch.cuda.synchronize()
    ret.check("returns"); adv.check("advantages")
    a = (d["rewards"], d["values"], d["dones"], d["last_values"], inp["gamma"], inp["lam"])
    (want, want_adv), (w32, a32) = R.gae(*a, F64), R.gae(*a, F32)
    R.check(f"gae {case[0]} returns", ret.t, want, w32)
    R.check(f"gae {case[0]} advantages", adv.t, want_adv, a32)
    assert torch.equal(adv.t, ret.t - d["values"]), "advantages are not returns - values in float32"
    for e in torch.nonzero(d["dones"][T - 1]).flatten().tolist()[:3]:        # done at T - 1: the env's own reward, last_values = 1e30 times zero
        assert float(d["last_values"][e]) == R.f32(R.HUGE)
        assert abs(float(ret.t[T - 1, e]) - float(d["rewards"][T - 1, e])) < R.bound(0.0, want)


def test_gae_through_the_storage():
    """RolloutStorage._gae_kernel (the [T, N, 1] storage, last_values [N, 1]) against the float64 restatement."""
    from legged_games_gym_amd.rl.ppo import RolloutStorage
    case = R.GAE_CASES[2]
    inp = R.gae_inputs(case)
    T, N = inp["T"], inp["N"]
    st = RolloutStorage(N, T, [4], [None], [2], device=DEV)
    d = _gae_device(inp)
    st.rewards.copy_(d["rewards"].unsqueeze(-1)); st.values.copy_(d["values"].unsqueeze(-1)); st.dones.copy_(d["dones"].unsqueeze(-1))
    st.returns.fill_(float("nan")); st.advantages.fill_(float("nan"))
    assert st._gae_kernel(d["last_values"].unsqueeze(-1), inp["gamma"], inp["lam"])
    a = (d["rewards"], d["values"], d["dones"], d["last_values"], inp["gamma"], inp["lam"])
    (want, want_adv), (w32, a32) = R.gae(*a, F64), R.gae(*a, F32)
    R.check("gae storage returns", st.returns[..., 0], want, w32)
    R.check("gae storage advantages", st.advantages[..., 0], want_adv, a32)


def test_gae_empty_sizes_write_nothing_and_a_null_pointer_is_refused():
    L = _lib()
    inp = R.gae_inputs(R.GAE_CASES[2])
    T, N = inp["T"], inp["N"]
    d = _gae_device(inp)
    ret, adv = Guarded((T, N), device=DEV), Guarded((T, N), device=DEV)
    p = [d["rewards"].data_ptr(), d["values"].data_ptr(), d["dones"].data_ptr(), d["last_values"].data_ptr()]
    assert L.lg_gae_returns(*p, 0.99, 0.95, ret.ptr(), adv.ptr(), 0, N, _stream()) == 0
    assert L.lg_gae_returns(*p, 0.99, 0.95, ret.ptr(), adv.ptr(), T, 0, _stream()) == 0
    for k in range(6):
        q = p + [ret.ptr(), adv.ptr()]
        q[k] = None
        _refused(L, L.lg_gae_returns(*q[:4], 0.99, 0.95, q[4], q[5], T, N, _stream()))
    torch.cuda.synchronize()
    assert ret.untouched() and adv.untouched()
    ret.check("returns"); adv.check("advantages")


# ------------------------------------------------------------------------------------------------ KL rule, clip, Adam
class AdamState:
    """Device copies of an Adam case between guard bands, the argument table of ``lg_adam_step`` and NaN-filled scratch."""

    def __init__(self, inp):
        from legged_games_gym_amd import capi
        g = lambda ts: [Guarded(t.shape, device=DEV, init=t.to(DEV)) for t in ts]
        self.params, self.exp_avg, self.exp_avg_sq = g(inp["params"]), g(inp["exp_avg"]), g(inp["exp_avg_sq"])
        self.steps = [Guarded(1, device=DEV, init=torch.tensor([s], device=DEV)) for s in inp["steps"]]
        self.grads = [t.to(DEV).contiguous() for t in inp["grads"]]
        self.lr = Guarded(1, device=DEV, init=torch.tensor([inp["lr"]], device=DEV))
        self.kl = None if inp["kl"] is None else torch.tensor([inp["kl"]], device=DEV)
        self.desired_kl = inp["desired_kl"]
        self.scratch = Guarded(capi.LG_ADAM_SCRATCH_FLOATS, device=DEV)
        self.n = len(self.params)
        self.table = (capi.lg_adam_tensor * self.n)()
        for i in range(self.n):
            e = self.table[i]
            e.param, e.grad, e.exp_avg, e.exp_avg_sq = self.params[i].ptr(), self.grads[i].data_ptr(), self.exp_avg[i].ptr(), self.exp_avg_sq[i].ptr()
            e.step, e.numel = self.steps[i].ptr(), self.params[i].t.numel()

    def set_grads(self, grads):
        for mine, new in zip(self.grads, grads):
            mine.copy_(new)

    def step(self, L, kl=None):
        if kl is not None:
            self.kl.fill_(kl)
        self.scratch.t.fill_(float("nan"))                      # stale partial sums must not leak
        return L.lg_adam_step(self.table, self.n, self.lr.ptr(), R.BETAS[0], R.BETAS[1], R.EPS, R.MAX_NORM, None if self.kl is None else self.kl.data_ptr(),
                              self.desired_kl, self.scratch.ptr(), _stream())

    def check_bands(self):
        torch.cuda.synchronize()
        for name in ("params", "exp_avg", "exp_avg_sq", "steps"):
            for k, b in enumerate(getattr(self, name)):
                b.check(f"{name}[{k}]")
        self.lr.check("lr"); self.scratch.check("scratch")

    def everything(self):
        return [b.t.clone() for name in ("params", "exp_avg", "exp_avg_sq", "steps") for b in getattr(self, name)] + [self.lr.t.clone(), self.scratch.t.clone()]


def _check_adam(label, S, want, want32):
    """Parameters, both moments (each over all tensors of the list at once), learning rate, norm and coefficient under the bound; steps exact."""
    p, m, v, steps, lr, norm, coef = want
    p32, m32, v32, _, lr32, norm32, coef32 = want32
    ratios = {"params": R.check(f"{label} params", _flat(b.t for b in S.params), _flat(p), _flat(p32)),
              "exp_avg": R.check(f"{label} exp_avg", _flat(b.t for b in S.exp_avg), _flat(m), _flat(m32)),
              "exp_avg_sq": R.check(f"{label} exp_avg_sq", _flat(b.t for b in S.exp_avg_sq), _flat(v), _flat(v32)),
              "lr": R.check(f"{label} lr", S.lr.t.cpu(), lr.reshape(1), lr32.reshape(1)),
              "norm": R.check(f"{label} norm", S.scratch.t[0:1].cpu(), norm.reshape(1), norm32.reshape(1)),
              "coef": R.check(f"{label} coef", S.scratch.t[1:2].cpu(), coef.reshape(1), coef32.reshape(1))}
    assert [float(b.t) for b in S.steps] == [float(s) for s in steps]
    return ratios


@pytest.mark.parametrize("case", R.ADAM_CASES, ids=R.ADAM_IDS)
def test_adam_kernels_match_float64_on_one_step(case):
    """One ``lg_adam_step`` from a synthetic optimiser state: tensor lists from one element to 32 tensors (a 1- and a 3-element tensor beside
    a 120 320-element one: 63 empty chunks each), step counts 0 .. 99 999 before the call, gradient norms on either side of max_norm and
    zero, every branch of the KL rule with its clamps and its strict comparisons.  Largest kernel / e32 on the MI355X: params 1.09, exp_avg 1.34 (the one-element tensor), exp_avg_sq 1.00, lr 1.00, norm 1.00, coef 1.00."""
    L = _lib()
    inp = R.adam_inputs(case)
    R.assert_adam_inputs(inp)
    S = AdamState(inp)
    rc = S.step(L)
    assert rc == 0, L.lg_last_error()
    S.check_bands()
    want, want32 = R.adam_restated(inp, F64), R.adam_restated(inp, F32)
    _check_adam("adam " + "-".join(str(x) for x in case), S, want, want32)
    if inp["grad_mode"] != "above":
        assert float(S.scratch.t[1]) == 1.0                     # not clipped: the coefficient is exactly 1
    if inp["kl_mode"] in ("equal", "zero", "on_upper", "on_lower", "null", "desired_zero"):
        assert float(S.lr.t) == inp["lr"], inp["kl_mode"]       # unchanged means untouched
    if inp["kl_mode"] == "above_clamped":
        assert float(S.lr.t) == R.f32(1e-5)
    if inp["kl_mode"] == "below_clamped":
        assert float(S.lr.t) == R.f32(1e-2)
    used = S.scratch.t[: 2 + 64 * S.n]
    assert bool(torch.isfinite(used).all()) and bool(torch.isnan(S.scratch.t[2 + 64 * S.n:]).all())


def test_adam_refuses_a_33rd_tensor_and_changes_nothing():
    L = _lib()
    inp = R.adam_inputs(("thirty_three", 9, "above", "above"))
    S = AdamState(inp)
    before = S.everything()
    _refused(L, S.step(L))
    S.check_bands()
    after = S.everything()
    assert all(torch.equal(a, b) for a, b in zip(before[:-1], after[:-1])) and S.scratch.untouched()
    _refused(L, L.lg_adam_step(S.table, 0, S.lr.ptr(), R.BETAS[0], R.BETAS[1], R.EPS, R.MAX_NORM, None, 0.0, S.scratch.ptr(), _stream()))
    S.n = 32                                                    # the first 32 of the same table are accepted
    assert S.step(L) == 0, L.lg_last_error()
    S.check_bands()
    assert float(S.steps[31].t) == 10.0 and float(S.steps[32].t) == 9.0 and torch.equal(S.params[32].t, before[32])


def test_adam_is_bit_reproducible():
    """Two calls from identical state give bit-identical results: the header promises a fixed summation order."""
    L = _lib()
    inp = R.adam_inputs(("small_beside_large", 9, "above", "above"))
    out = []
    for _ in range(2):
        S = AdamState(inp)
        assert S.step(L) == 0, L.lg_last_error()
        S.check_bands()
        out.append(S.everything())
    nan_equal = lambda a, b: torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0))
    assert all(nan_equal(a, b) for a, b in zip(*out))


def test_adam_200_calls_match_200_float64_steps():
    """200 calls on the tensors of one 48-128-64-32 network, gradients alternating between size 3 and 0.01, the KL statistic cycling over
    0.05 / 0.001 / 0.01 with the learning rate carried on the device, against 200 float64 steps under the same rule; e32 is the drift of
    the float32 restatement over the same 200 steps.  Largest kernel / e32 on the MI355X: params 1.00, exp_avg 0.78, exp_avg_sq 1.00, lr bit-equal to the float32 restatement."""
    L = _lib()
    inp = R.adam_inputs(("flat_48_128_64_32", 0, "above", "above"))
    shapes = R.ADAM_LISTS["flat_48_128_64_32"]
    S = AdamState(inp)
    g = torch.Generator().manual_seed(9)
    state = {d: (inp["params"], inp["exp_avg"], inp["exp_avg_sq"], inp["steps"], inp["lr"]) for d in (F64, F32)}
    for it in range(200):
        grads = R.sequence_gradients(shapes, it, g)
        kl = R.f32(R.SEQUENCE_KL[it % 3])
        S.set_grads(grads)
        assert S.step(L, kl=kl) == 0, L.lg_last_error()
        for d in (F64, F32):
            p, m, v, steps, lr = state[d]
            state[d] = R.adam_step(p, grads, m, v, steps, lr, R.BETAS, R.EPS, R.MAX_NORM, kl, R.DESIRED_KL, d)[:5]
    S.check_bands()
    p, m, v, steps, lr = state[F64]
    p32, m32, v32, _, lr32 = state[F32]
    R.check("adam 200 calls params", _flat(b.t for b in S.params), _flat(p), _flat(p32))
    R.check("adam 200 calls exp_avg", _flat(b.t for b in S.exp_avg), _flat(m), _flat(m32))
    R.check("adam 200 calls exp_avg_sq", _flat(b.t for b in S.exp_avg_sq), _flat(v), _flat(v32))
    R.check("adam 200 calls lr", S.lr.t.cpu(), lr.reshape(1), lr32.reshape(1))
    assert [float(b.t) for b in S.steps] == [200.0] * len(shapes) == [float(s) for s in steps]
    assert max(R.err(a, b) for a, b in zip(p, inp["params"])) > 0.01      # the parameters did move


# ------------------------------------------------------------------------------------------------ lg_rollout_record
class RecordRun:
    """Device buffers of T consecutive ``lg_rollout_record`` calls on the transitions ``inp``: storage [T, ...] between guard bands, NaN-filled;
    the running statistics between guard bands."""

    def __init__(self, inp, N, O, A, T, form):
        self.N, self.O, self.A, self.T = N, O, A, T
        self.use_std, self.t_in, self.t_out, self.stats = form
        self.d = {k: (v.to(DEV).contiguous() if v is not None else None) for k, v in inp.items()}
        G = lambda *s, dtype=F32: Guarded(s, dtype=dtype, device=DEV)
        self.st = dict(obs=G(T, N, O), actions=G(T, N, A), mu=G(T, N, A), rewards=G(T, N), dones=G(T, N, dtype=torch.uint8), time_outs=G(T, N), sigma=G(T, N, A),
                       log_prob=G(T, N))
        self.cur_return = Guarded(N, device=DEV, init=self.d["cur_return"])
        self.cur_length = Guarded(N, device=DEV, init=self.d["cur_length"])
        self.sums = Guarded(3, device=DEV, init=self.d["sums"])

    def struct(self, t):
        from legged_games_gym_amd import capi
        s, d, st = capi.lg_rollout_step(), self.d, self.st
        s.num_envs, s.num_obs, s.num_actions = self.N, self.O, self.A
        s.obs, s.actions, s.mean, s.rewards, s.dones = (d[k][t].data_ptr() for k in ("obs", "actions", "mean", "rewards", "dones"))
        s.time_outs = d["time_outs"][t].data_ptr() if self.t_in else None
        s.storage_obs, s.storage_actions, s.storage_mu, s.storage_rewards, s.storage_dones = (st[k].t[t].data_ptr() for k in ("obs", "actions", "mu", "rewards", "dones"))
        s.storage_time_outs = st["time_outs"].t[t].data_ptr() if self.t_out else None
        if self.use_std:
            s.std, s.storage_sigma, s.storage_log_prob = d["std"].data_ptr(), st["sigma"].t[t].data_ptr(), st["log_prob"].t[t].data_ptr()
        if self.stats:
            s.cur_return, s.cur_length, s.sums = self.cur_return.ptr(), self.cur_length.ptr(), self.sums.ptr()
        return s

    def check_bands(self):
        torch.cuda.synchronize()
        for k, b in self.st.items():
            b.check(k)
        self.cur_return.check("cur_return"); self.cur_length.check("cur_length"); self.sums.check("sums")

    def outputs_untouched(self):
        return all(b.untouched() for b in self.st.values())


def _restate_steps(inp, T, form, dtype):
    """T record steps through the restatement at ``dtype``, the statistics carried -> (per-step dicts, cur_return, cur_length, sums, terms)."""
    use_std, t_in, t_out, stats = form
    cr, cl, sums = (inp["cur_return"], inp["cur_length"], inp["sums"]) if stats else (None, None, None)
    outs, terms = [], []
    for t in range(T):
        o = R.record(inp["obs"][t], inp["actions"][t], inp["mean"][t], inp["rewards"][t], inp["dones"][t], inp["time_outs"][t] if t_in else None,
                     inp["std"] if use_std else None, cr, cl, sums, dtype)
        if stats:
            cr, cl, sums = o["cur_return"], o["cur_length"], o["sums"]
            terms.append(o["terms"])
        outs.append(o)
    return outs, cr, cl, sums, (torch.cat(terms) if stats else None)


def _check_statistics(label, cur_return, cur_length, sums, w64, w32):
    """Running return under the bound and bit-equal to the float32 restatement (one float32 add per step, in step order: nothing to contract
    or reorder), running length and sums[1:] exact.  sums[0]: the terms the kernel adds are therefore the float32 restatement's ended
    returns, bit for bit; its atomics add them to the starting value in any order, and the result is held to the summation bound against
    the float64 sum of those same float32 terms."""
    (cr, cl, s, terms), (cr32, cl32, s32, terms32) = w64, w32
    R.check(f"{label} cur_return", cur_return.cpu(), cr, cr32)
    assert torch.equal(cur_return.cpu(), cr32), "the running return is not the float32 sum in step order"
    assert torch.equal(cur_length.cpu().double(), cl) and torch.equal(cl32.double(), cl)
    assert float(sums[1]) == float(s[1]) and float(sums[2]) == float(s[2]) and float(s[1]) < 2 ** 24
    x = torch.cat((torch.tensor([R.SUMS0[0]]), terms32))
    want0 = float(x.double().sum())
    b = R.sum_bound(x, want0)
    e = abs(float(sums[0]) - want0)
    print(f"[observed] {label} sums[0]: kernel {e:.3e}  bound {b:.3e}  terms {x.numel()}  (float64 restatement {abs(float(s[0]) - want0):.3e} from the sum of the float32 terms)")
    assert e <= b, (e, b)


@pytest.mark.parametrize("form", list(R.RECORD_FORMS))
@pytest.mark.parametrize("case", R.RECORD_CASES, ids=str)
def test_rollout_record_kernel_matches_float64(case, form):
    """Three consecutive steps in every call form the runners use, from one env with two actions to 16 actions and num_actions == num_obs.
    Largest kernel / e32 on the MI355X: log_prob 2.29 (17 envs, 3 actions; 0.9 .. 1.1 from 12 actions), cur_return 1.00;
    sums[0] at most 0.24 of its bound (one env, 3 terms)."""
    L = _lib()
    N, O, A = case
    T, f = R.RECORD_STEPS, R.RECORD_FORMS[form]
    use_std, t_in, t_out, stats = f
    inp = R.record_inputs(case)
    R.assert_record_inputs(case, inp)
    run = RecordRun(inp, N, O, A, T, f)
    for t in range(T):
        assert L.lg_rollout_record(run.struct(t), _stream()) == 0, L.lg_last_error()
    run.check_bands()
    st = {k: b.t.cpu() for k, b in run.st.items()}
    assert torch.equal(st["obs"], inp["obs"]) and torch.equal(st["actions"], inp["actions"]) and torch.equal(st["mu"], inp["mean"])
    assert torch.equal(st["rewards"], inp["rewards"]) and torch.equal(st["dones"], inp["dones"])
    w64, w32 = _restate_steps(inp, T, f, F64), _restate_steps(inp, T, f, F32)
    label = f"record {case} {form}"
    if t_out:
        assert torch.equal(st["time_outs"], torch.stack([o["time_outs"] for o in w64[0]]))
        assert bool(st["time_outs"].any()) == (t_in and bool(inp["time_outs"].any()))
    else:
        assert run.st["time_outs"].untouched()
    if use_std:
        assert torch.equal(st["sigma"], inp["std"].expand(T, N, A))                                  # a bit copy of std
        R.check(f"{label} log_prob", st["log_prob"], torch.stack([o["log_prob"] for o in w64[0]]), torch.stack([o["log_prob"] for o in w32[0]]))
    else:
        assert run.st["sigma"].untouched() and run.st["log_prob"].untouched()                        # handed to nobody
    if stats:
        _check_statistics(label, run.cur_return.t, run.cur_length.t, run.sums.t, w64[1:], w32[1:])
    else:
        assert torch.equal(run.cur_return.t.cpu(), inp["cur_return"]) and torch.equal(run.cur_length.t.cpu(), inp["cur_length"]) and torch.equal(run.sums.t.cpu(), inp["sums"])


def test_rollout_record_refusals_write_nothing():
    L = _lib()
    case = R.RECORD_CASES[2]
    N, O, A = case
    inp = R.record_inputs(case)
    run = RecordRun(inp, N, O, A, R.RECORD_STEPS, R.RECORD_FORMS["legged"])

    def more_actions_than_observations(s):
        s.num_actions, s.num_obs = 4, 3

    def seventeen_actions(s):
        s.num_actions, s.num_obs = 17, 20

    def std_without_its_storages(s):
        s.storage_sigma = None

    def std_without_log_prob(s):
        s.storage_log_prob = None

    def return_without_length(s):
        s.cur_length = None

    def length_without_return(s):
        s.cur_return = None

    for spoil in (more_actions_than_observations, seventeen_actions, std_without_its_storages, std_without_log_prob, return_without_length, length_without_return):
        s = run.struct(0)
        spoil(s)
        _refused(L, L.lg_rollout_record(s, _stream()))
    run.check_bands()
    assert run.outputs_untouched()
    assert torch.equal(run.cur_return.t.cpu(), inp["cur_return"]) and torch.equal(run.cur_length.t.cpu(), inp["cur_length"]) and torch.equal(run.sums.t.cpu(), inp["sums"])


# ------------------------------------------------------------------------------------------------ lg_rollout_finish
def _finish_struct(d, out, stats, lo, hi, N, A, t_in, t_out, with_stats):
    from legged_games_gym_amd import capi
    s = capi.lg_rollout_post()
    s.steps, s.num_envs, s.num_actions = hi - lo, N, A
    s.actions, s.mean, s.rewards, s.dones, s.std = d["actions"][lo:].data_ptr(), d["mean"][lo:].data_ptr(), d["rewards"][lo:].data_ptr(), d["dones"][lo:].data_ptr(), d["std"].data_ptr()
    s.time_outs = d["time_outs"][lo:].data_ptr() if t_in else None
    s.sigma, s.log_prob = out["sigma"].t[lo:].data_ptr(), out["log_prob"].t[lo:].data_ptr()
    s.time_outs_f = out["time_outs"].t[lo:].data_ptr() if t_out else None
    if with_stats:
        s.cur_return, s.cur_length, s.sums = (b.ptr() for b in stats)
    return s


@pytest.mark.parametrize("variant", list(R.FINISH_VARIANTS))
@pytest.mark.parametrize("case", R.FINISH_CASES, ids=str)
def test_rollout_finish_kernel_matches_float64(case, variant):
    """Two consecutive segments over the same running statistics (episodes span the boundary) against the float64 restatement; in all cases
    but the last, T N 16 is no multiple of 256, so the clamped tail lanes of the last transition workgroup run.  In the full variant the
    same data fed step by step to ``lg_rollout_record`` gives the same exact quantities and log-probs within the bound.
    Largest kernel / e32 on the MI355X: log_prob 2.10 (one env, 2 actions; 0.95 at 12 and 0.99 at 16 actions), cur_return 1.00; sums[0] at most
    0.11 of its bound (one env, 2 terms); the log-probs of the two kernels were bit-identical in all five cases."""
    L = _lib()
    T, N, A = case
    t_in, t_out, with_stats = R.FINISH_VARIANTS[variant]
    inp = R.finish_inputs(case)
    R.assert_finish_inputs(case, inp)
    d = {k: (v.to(DEV).contiguous() if v is not None else None) for k, v in inp.items()}
    out = dict(sigma=Guarded((2 * T, N, A), device=DEV), log_prob=Guarded((2 * T, N), device=DEV), time_outs=Guarded((2 * T, N), device=DEV))
    stats = [Guarded(N, device=DEV, init=d["cur_return"]), Guarded(N, device=DEV, init=d["cur_length"]), Guarded(3, device=DEV, init=d["sums"])]
    for seg in range(2):
        s = _finish_struct(d, out, stats, seg * T, (seg + 1) * T, N, A, t_in, t_out, with_stats)
        assert L.lg_rollout_finish(s, _stream()) == 0, L.lg_last_error()
    torch.cuda.synchronize()
    for k, b in out.items():
        b.check(k)
    for b in stats:
        b.check("statistics")

    def restate(dtype):
        cr, cl, sums = (inp["cur_return"], inp["cur_length"], inp["sums"]) if with_stats else (None, None, None)
        segs, terms = [], []
        for seg in range(2):
            sl = slice(seg * T, (seg + 1) * T)
            o = R.finish(inp["actions"][sl], inp["mean"][sl], inp["rewards"][sl], inp["dones"][sl], inp["time_outs"][sl] if t_in else None, inp["std"], cr, cl, sums, dtype)
            if with_stats:
                cr, cl, sums = o["cur_return"], o["cur_length"], o["sums"]
                terms.append(o["terms"])
            segs.append(o)
        return segs, cr, cl, sums, (torch.cat(terms) if with_stats else None)
    w64, w32 = restate(F64), restate(F32)
    label = f"finish {case} {variant}"
    assert torch.equal(out["sigma"].t.cpu(), inp["std"].expand(2 * T, N, A))
    lp = out["log_prob"].t.cpu()
    R.check(f"{label} log_prob", lp, torch.cat([o["log_prob"] for o in w64[0]]), torch.cat([o["log_prob"] for o in w32[0]]))
    if t_out:
        assert torch.equal(out["time_outs"].t.cpu(), torch.cat([o["time_outs"] for o in w64[0]]))
        assert bool(out["time_outs"].t.any()) == (t_in and bool(inp["time_outs"].any()))
    else:
        assert out["time_outs"].untouched()
    if with_stats:
        _check_statistics(label, stats[0].t, stats[1].t, stats[2].t, w64[1:], w32[1:])
    else:
        assert torch.equal(stats[0].t.cpu(), inp["cur_return"]) and torch.equal(stats[1].t.cpu(), inp["cur_length"]) and torch.equal(stats[2].t.cpu(), inp["sums"])
    if variant != "full":
        return
    # the same data step by step through lg_rollout_record (the observation slot is fed the means: num_obs = num_actions)
    rec_inp = dict(inp, obs=inp["mean"])
    run = RecordRun(rec_inp, N, A, A, 2 * T, R.RECORD_FORMS["legged"])
    for t in range(2 * T):
        assert L.lg_rollout_record(run.struct(t), _stream()) == 0, L.lg_last_error()
    run.check_bands()
    assert torch.equal(run.st["sigma"].t, out["sigma"].t) and torch.equal(run.st["time_outs"].t, out["time_outs"].t)
    assert torch.equal(run.cur_length.t, stats[1].t) and torch.equal(run.cur_return.t, stats[0].t)          # one float32 add per step, in step order, in both
    assert torch.equal(run.sums.t[1:], stats[2].t[1:])
    rec_lp = run.st["log_prob"].t.cpu()
    print(f"[observed] {label}: log-probs of lg_rollout_record and lg_rollout_finish bit-identical: {torch.equal(rec_lp, lp)}")
    R.check(f"{label} log_prob of lg_rollout_record", rec_lp, torch.cat([o["log_prob"] for o in w64[0]]), torch.cat([o["log_prob"] for o in w32[0]]))


def test_rollout_finish_refusals_write_nothing():
    L = _lib()
    case = R.FINISH_CASES[1]
    T, N, A = case
    inp = R.finish_inputs(case)
    d = {k: (v.to(DEV).contiguous() if v is not None else None) for k, v in inp.items()}
    out = dict(sigma=Guarded((2 * T, N, A), device=DEV), log_prob=Guarded((2 * T, N), device=DEV), time_outs=Guarded((2 * T, N), device=DEV))
    stats = [Guarded(N, device=DEV, init=d["cur_return"]), Guarded(N, device=DEV, init=d["cur_length"]), Guarded(3, device=DEV, init=d["sums"])]

    def seventeen_actions(s):
        s.num_actions = 17

    def no_steps(s):
        s.steps = 0

    def no_std(s):
        s.std = None

    def return_without_length(s):
        s.cur_length = None

    for spoil in (seventeen_actions, no_steps, no_std, return_without_length):
        s = _finish_struct(d, out, stats, 0, T, N, A, True, True, True)
        spoil(s)
        _refused(L, L.lg_rollout_finish(s, _stream()))
    torch.cuda.synchronize()
    assert all(b.untouched() for b in out.values())
    assert torch.equal(stats[0].t.cpu(), inp["cur_return"]) and torch.equal(stats[2].t.cpu(), inp["sums"])
