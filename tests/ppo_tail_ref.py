"""Shared pieces of tests/test_gpu_ppo_tail.py (GPU) and tests/test_ppo_tail_ref.py (CPU): plain torch restatements of the tail of a PPO
iteration -- the GAE scan, the KL rule + gradient clip + Adam, the rollout bookkeeping per step and per segment -- that take a ``dtype``,
the tolerance rule the GPU tests assert with, guard-banded buffers, and the cases both files run with their seeded inputs.

The restatements are written from the reference's formulas (rsl_rl ``RolloutStorage.compute_returns``, ``PPO.act`` /
``process_env_step``, the tail of ``PPO.update``, ``OnPolicyRunner.learn``'s ``rewbuffer`` / ``lenbuffer``), not from the kernels.
Nothing here touches the device library, so everything in this file is tested without a GPU."""
import math

import torch

F32, F64 = torch.float32, torch.float64
ULP = 2.0 ** -23          # spacing of float32 at 1 (the floor of the tolerance rule)
UNIT = 2.0 ** -24         # unit roundoff of float32 (the summation bound)


# ------------------------------------------------------------------------------------------------ the tolerance rule
def bound(e32, want, margin=4.0):
    """Largest admissible |kernel - want|: ``margin`` x the larger of ``e32`` (max |float32 restatement - want| on the same inputs) and
    one float32 spacing at max |want|.  4: FMA contraction, 1-ulp divide / square root and __logf are each worth a few units in the last
    place and e32, a maximum over a sample, moves by about 2x with the seed; the floor keeps a lucky e32 from giving an impossible bound."""
    return margin * max(float(e32), ULP * float(want.detach().abs().max()) if want.numel() else 0.0)


def err(a, b):
    """max |a - b| in float64 on the CPU (0 for empty tensors)."""
    if a.numel() == 0:
        assert b.numel() == 0
        return 0.0
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def check(label, got, want, want32, margin=4.0, out=print):
    """THE float comparison of the tail tests: ``got`` (kernel, float32) against ``want`` (restatement at float64) under ``bound`` with
    e32 measured from ``want32`` (restatement at float32).  Prints the figures as ``[observed]`` and returns kernel error / e32."""
    assert got.shape == want.shape == want32.shape, f"{label}: shapes {tuple(got.shape)} {tuple(want.shape)} {tuple(want32.shape)}"
    assert bool(torch.isfinite(got).all()), f"{label}: {int((~torch.isfinite(got)).sum())} non-finite elements (not overwritten?)"
    e, e32 = err(got, want), err(want32, want)
    b = bound(e32, want, margin)
    ratio = e / e32 if e32 > 0.0 else (0.0 if e == 0.0 else float("inf"))
    out(f"[observed] {label}: kernel {e:.3e}  e32 {e32:.3e}  bound {b:.3e}  kernel/e32 {ratio:.2f}  max|want| {float(want.abs().max()) if want.numel() else 0.0:.3e}")
    assert e < b or (e == 0.0 and b == 0.0), f"{label}: max error {e:.3e} >= bound {b:.3e} (e32 {e32:.3e}, margin {margin:g})"
    return ratio


def sum_bound(terms32, result):
    """Bound on |float32 sum of ``terms32`` accumulated in ANY order - their float64 sum| (the atomically accumulated ``sums[0]``):
    (n - 1) 2^-24 sum |x_i| over the n terms added (the starting value included), plus one float32 spacing at ``result``."""
    x = terms32.double()
    r = abs(float(result))
    ulp = 2.0 ** (math.floor(math.log2(r)) - 23) if r > 0.0 else 2.0 ** -149
    return (x.numel() - 1) * UNIT * float(x.abs().sum()) + ulp


# ------------------------------------------------------------------------------------------------ guard bands
GUARD = 64


class Guarded:
    """A buffer with ``GUARD`` sentinel elements on either side of the view a kernel is handed (``.t``).  ``check()`` asserts that the
    bands are as they were made.  Floats: sentinel -7777, inside NaN unless ``init`` is given; bytes: sentinel 0xA5, inside 0xFF."""
    SENTINEL = {torch.float32: -7777.0, torch.uint8: 0xA5, torch.float64: -7777.0}

    def __init__(self, shape, dtype=F32, device="cpu", init=None):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = int(math.prod(shape))
        self.n, self.sentinel = n, self.SENTINEL[dtype]
        self.buf = torch.full((n + 2 * GUARD,), self.sentinel, dtype=dtype, device=device)
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        if init is not None:
            self.t.copy_(init)
        else:
            self.t.fill_(0xFF if dtype == torch.uint8 else float("nan"))

    def ptr(self):
        return self.t.data_ptr()

    def check(self, label=""):
        lo, hi = self.buf[:GUARD], self.buf[GUARD + self.n:]
        assert bool((lo == self.sentinel).all()), f"{label}: the band below the buffer was written"
        assert bool((hi == self.sentinel).all()), f"{label}: the band above the buffer was written"

    def untouched(self):
        """The inside is still as an uninitialised one was made (all NaN / all 0xFF)."""
        return bool(torch.isnan(self.t).all()) if self.t.is_floating_point() else bool((self.t == 0xFF).all())


# ------------------------------------------------------------------------------------------------ GAE
def gae(rewards, values, dones, last_values, gamma, lam, dtype):
    """rsl_rl RolloutStorage.compute_returns without the normalisation: [T, N] rewards / values / dones, [N] last_values ->
    (returns, advantages), advantages = returns - values."""
    r, v, lv = rewards.to(dtype), values.to(dtype), last_values.to(dtype)
    T = r.shape[0]
    returns = torch.empty_like(r)
    advantage = torch.zeros_like(lv)
    for step in reversed(range(T)):
        next_values = lv if step == T - 1 else v[step + 1]
        next_is_not_terminal = 1.0 - dones[step].to(dtype)
        delta = r[step] + next_is_not_terminal * gamma * next_values - v[step]
        advantage = delta + next_is_not_terminal * gamma * lam * advantage
        returns[step] = advantage + v[step]
    return returns, returns - v


# (id, T, N, gamma, lam, value scale, reward scale)
GAE_CASES = [
    ("T1_N1", 1, 1, 0.99, 0.95, 0.3, 0.02),
    ("T1_N257", 1, 257, 0.99, 0.95, 0.3, 0.02),
    ("T24_N255", 24, 255, 0.99, 0.95, 0.3, 0.02),
    ("T24_N256", 24, 256, 0.99, 0.95, 0.3, 0.02),
    ("T24_N777", 24, 777, 0.99, 0.95, 0.3, 0.02),
    ("T100_N300_long_memory", 100, 300, 0.999, 0.99, 0.3, 0.02),
    ("T64_N257_large_values", 64, 257, 0.99, 0.95, 30.0, 1.0),
]
GAE_IDS = [c[0] for c in GAE_CASES]
HUGE = 1e30               # last_values of an env that is done at T - 1: finite, and must be multiplied by zero


def gae_inputs(case):
    """Seeded CPU inputs of a GAE case.  Env 0 has no done, env 1 a done on every step, env 2 its only done at T - 1 (from N >= 3); the
    others draw dones at 4 %.  An env whose last step is done gets last_values = HUGE.  N = 1: the env is done at T - 1."""
    name, T, N, gamma, lam, vs, rs = case
    g = torch.Generator().manual_seed(1000 + 7 * T + N)
    rewards = torch.randn(T, N, generator=g) * rs
    values = torch.randn(T, N, generator=g) * vs
    last = torch.randn(N, generator=g) * vs
    dones = (torch.rand(T, N, generator=g) < 0.04).to(torch.uint8)
    if N >= 3:
        dones[:, 0] = 0
        dones[:, 1] = 1
        dones[:, 2] = 0
        dones[T - 1, 2] = 1
    else:
        dones[T - 1, 0] = 1
    last[dones[T - 1] != 0] = HUGE
    return dict(rewards=rewards, values=values, dones=dones, last_values=last, gamma=gamma, lam=lam, T=T, N=N)


def assert_gae_inputs(inp):
    """The done patterns the GAE tests rely on, on the inputs alone."""
    d, T, N = inp["dones"], inp["T"], inp["N"]
    per_env = d.sum(0)
    last_done = d[T - 1] != 0
    assert bool(last_done.any()) and bool((inp["last_values"][last_done] == HUGE).all()) and bool(torch.isfinite(inp["last_values"]).all())
    assert bool((inp["last_values"][~last_done].abs() < 1e3).all())
    if N >= 3:
        assert bool((per_env == 0).any()), "no env without a done"
        assert bool((per_env == T).any()), "no env with a done on every step"
        assert bool(((per_env == 1) & last_done).any()) or T == 1, "no env with its only done at T - 1"
    if T * N >= 255:
        share = float(d.float().mean())
        assert 0.01 <= share <= 0.10, share


# ------------------------------------------------------------------------------------------------ KL rule, clip, Adam
def adam_step(params, grads, exp_avg, exp_avg_sq, steps, lr, betas, eps, max_norm, kl, desired_kl, dtype):
    """The tail of rsl_rl PPO.update's mini-batch step in the reference's order: the KL rule on ``lr``; clip_grad_norm_ over all tensors
    together; torch.optim.Adam (no weight decay, no amsgrad) with the bias corrections of the incremented step.  Lists of tensors, ``steps``
    a list of numbers, ``lr`` / ``kl`` numbers (``kl`` None: fixed schedule).  The thresholds 2 d and d / 2 are formed from float32(d), so
    a ``kl`` placed exactly on one compares the same way at either dtype.  -> (params, exp_avg, exp_avg_sq, steps, lr, norm, coef)."""
    c = lambda x: torch.as_tensor(x, dtype=F64).to(dtype) if not torch.is_tensor(x) else x.detach().to(dtype)
    lr = c(lr)
    if kl is not None and desired_kl > 0:
        d32 = float(torch.tensor(desired_kl, dtype=F32))
        if kl > 2.0 * d32:
            lr = torch.clamp(lr / 1.5, min=1e-5)
        elif kl < 0.5 * d32 and kl > 0.0:
            lr = torch.clamp(lr * 1.5, max=1e-2)
    g = [c(x) for x in grads]
    norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(x) for x in g]))
    coef = torch.clamp(c(max_norm) / (norm + 1e-6), max=1.0)
    beta1, beta2 = c(betas[0]), c(betas[1])
    new_p, new_m, new_v, new_steps = [], [], [], []
    for p, x, m, v, step in zip(params, g, exp_avg, exp_avg_sq, steps):
        p, m, v = c(p), c(m), c(v)
        x = x * coef
        step = step + 1
        m = m + (x - m) * (1 - beta1)                                  # exp_avg.lerp_(grad, 1 - beta1)
        v = v * beta2 + (1 - beta2) * x * x                            # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        bias_correction1 = 1 - beta1 ** c(step)
        bias_correction2 = 1 - beta2 ** c(step)
        step_size = lr / bias_correction1
        denom = v.sqrt() / bias_correction2.sqrt() + eps
        new_p.append(p - step_size * (m / denom))
        new_m.append(m); new_v.append(v); new_steps.append(step)
    return new_p, new_m, new_v, new_steps, lr, norm, coef


def mlp_shapes(dims):
    return [s for a, b in zip(dims[:-1], dims[1:]) for s in ((b, a), (b,))]


def recurrent_shapes(num_obs=48, hidden=256, mlp=(256, 256, 256), actions=12):
    """Parameter shapes of ActorCriticRecurrent in module order: std, actor, critic, the two LSTM memories (weight_ih, weight_hh, two biases)."""
    lstm = [(4 * hidden, num_obs), (4 * hidden, hidden), (4 * hidden,), (4 * hidden,)]
    return [(actions,)] + mlp_shapes([hidden, *mlp, actions]) + mlp_shapes([hidden, *mlp, 1]) + lstm + lstm


ADAM_LISTS = {
    "one_element": [(1,)],
    "small_beside_large": [(1,), (3,), (255,), (256,), (257,), (512, 235)],        # 120 320: chunk_len 1880 divides none of them
    "game_actor_critic": [(6,)] + mlp_shapes([19, 512, 256, 128, 6]) + mlp_shapes([19, 512, 256, 128, 1]),
    "recurrent": recurrent_shapes(),
    "thirty_two": [((k * 37) % 300 + 1,) if k % 5 else (64, 17 + k) for k in range(32)],
    "thirty_three": [(k + 1,) for k in range(33)],
    "flat_48_128_64_32": mlp_shapes([48, 128, 64, 32, 12]),
}
assert len(ADAM_LISTS["game_actor_critic"]) == 17 and len(ADAM_LISTS["recurrent"]) == 25 and len(ADAM_LISTS["thirty_two"]) == 32
MAX_NORM, DESIRED_KL, BETAS, EPS = 1.0, 0.01, (0.9, 0.999), 1e-8
D32 = float(torch.tensor(DESIRED_KL, dtype=F32))
# name -> (kl or None, lr before, desired_kl, lr after as a function of lr before)
KL_MODES = {
    "above": (0.05, 1e-3, DESIRED_KL, lambda lr: lr / 1.5),
    "above_clamped": (0.05, 1.2e-5, DESIRED_KL, lambda lr: 1e-5),
    "below": (0.001, 1e-3, DESIRED_KL, lambda lr: lr * 1.5),
    "below_clamped": (0.001, 8e-3, DESIRED_KL, lambda lr: 1e-2),
    "equal": (0.01, 1e-3, DESIRED_KL, lambda lr: lr),
    "zero": (0.0, 1e-3, DESIRED_KL, lambda lr: lr),
    "on_upper": (2.0 * D32, 1e-3, DESIRED_KL, lambda lr: lr),
    "on_lower": (0.5 * D32, 1e-3, DESIRED_KL, lambda lr: lr),
    "null": (None, 1e-3, DESIRED_KL, lambda lr: lr),
    "desired_zero": (0.05, 1e-3, 0.0, lambda lr: lr),
}
GRAD_NORMS = {"below": 0.5, "above": 3.0, "zero": 0.0}
STEP_COUNTS = (0, 1, 9, 999, 99999)
# (tensor list, step count before the call, gradient mode, KL mode): every list, every step count, every gradient mode and every KL mode
ADAM_CASES = ([(l, s, gm, km) for l, s, gm, km in (
    ("one_element", 0, "above", "above"), ("one_element", 9, "below", "null"), ("one_element", 99999, "zero", "zero"),
    ("small_beside_large", 1, "above", "below"), ("small_beside_large", 999, "below", "above_clamped"), ("small_beside_large", 0, "zero", "equal"),
    ("game_actor_critic", 9, "above", "below_clamped"), ("game_actor_critic", 99999, "below", "on_upper"),
    ("recurrent", 999, "above", "on_lower"), ("recurrent", 0, "below", "desired_zero"),
    ("thirty_two", 1, "above", "above"), ("thirty_two", 99999, "below", "below"))]
    + [("flat_48_128_64_32", s, "above", "equal") for s in STEP_COUNTS]
    + [("flat_48_128_64_32", 9, "below", km) for km in KL_MODES])
ADAM_IDS = ["-".join(str(x) for x in c) for c in ADAM_CASES]


def f32(x):
    """A number rounded to float32 (what a float32 device scalar holds)."""
    return float(torch.tensor(x, dtype=F32))


def adam_inputs(case):
    """Seeded CPU float32 state of an Adam case: parameters of size <= 1e-2, exp_avg_sq positive over 1e-12 .. 1, exp_avg within
    sqrt(exp_avg_sq), gradients scaled so that their float64 norm over all tensors is GRAD_NORMS[mode]."""
    name, step, grad_mode, kl_mode = case
    shapes = ADAM_LISTS[name]
    g = torch.Generator().manual_seed(77 + 13 * len(shapes) + step % 1000)
    params = [(torch.rand(s, generator=g) * 2 - 1) * 1e-2 for s in shapes]
    v = [10.0 ** (-12.0 * torch.rand(s, generator=g)) for s in shapes]
    m = [(torch.rand(s, generator=g) * 2 - 1) * x.sqrt() for s, x in zip(shapes, v)]
    grads = [torch.randn(s, generator=g) for s in shapes]
    total = math.sqrt(sum(float(x.double().square().sum()) for x in grads))
    grads = [(x.double() * (GRAD_NORMS[grad_mode] / total)).float() for x in grads]
    kl, lr, desired, after = KL_MODES[kl_mode]
    return dict(params=params, grads=grads, exp_avg=m, exp_avg_sq=v, steps=[float(step)] * len(shapes), lr=f32(lr), kl=None if kl is None else f32(kl),
                desired_kl=desired, lr_after=after, grad_mode=grad_mode, kl_mode=kl_mode)


def assert_adam_inputs(inp):
    norm = math.sqrt(sum(float(x.double().square().sum()) for x in inp["grads"]))
    mode = inp["grad_mode"]
    assert abs(norm - MAX_NORM) >= 0.01 * MAX_NORM, norm
    assert (norm == 0.0) if mode == "zero" else ((norm < MAX_NORM) == (mode == "below")), (mode, norm)
    assert all(float(p.abs().max()) <= 1e-2 for p in inp["params"])
    v = torch.cat([x.flatten() for x in inp["exp_avg_sq"]])
    assert float(v.min()) > 0.0 and float(v.max()) <= 1.0 and (v.numel() < 100 or (float(v.min()) < 1e-10 and float(v.max()) > 1e-2))
    if inp["kl_mode"] in ("on_upper", "on_lower"):
        assert inp["kl"] in (2.0 * D32, 0.5 * D32)                      # representable: the comparison is decided by strictness alone


def adam_restated(inp, dtype):
    return adam_step(inp["params"], inp["grads"], inp["exp_avg"], inp["exp_avg_sq"], inp["steps"], inp["lr"], BETAS, EPS, MAX_NORM, inp["kl"],
                     inp["desired_kl"], dtype)


def sequence_gradients(shapes, it, generator):
    """Gradients of call ``it`` of the 200-call sequence: size 3 on odd calls, 0.01 on even ones (tests/test_gpu_rl.py's alternation)."""
    return [torch.randn(s, generator=generator) * (3.0 if it % 2 else 0.01) for s in shapes]


SEQUENCE_KL = (0.05, 0.001, 0.01)


# ------------------------------------------------------------------------------------------------ rollout bookkeeping
def log_prob(actions, mean, std, dtype):
    """torch.distributions.Normal(mean, std).log_prob(actions).sum(-1) written out (PPO.act's actions_log_prob)."""
    a, m, s = actions.to(dtype), mean.to(dtype), std.to(dtype)
    var = s ** 2
    return (-((a - m) ** 2) / (2 * var) - s.log() - math.log(math.sqrt(2 * math.pi))).sum(-1)


def episode_step(cur_return, cur_length, rewards, dones, dtype):
    """OnPolicyRunner.learn's bookkeeping of one env step: cur_reward_sum += rewards, cur_episode_length += 1, the sums / lengths of the envs
    that ended go to rewbuffer / lenbuffer and are zeroed.  -> (cur_return, cur_length, ended returns, ended lengths)."""
    cr, cl = cur_return.to(dtype) + rewards.to(dtype), cur_length.to(dtype) + 1
    ended = dones != 0
    er, el = cr[ended], cl[ended]
    cr, cl = cr.clone(), cl.clone()
    cr[ended] = 0
    cl[ended] = 0
    return cr, cl, er, el


def record(obs, actions, mean, rewards, dones, time_outs, std, cur_return, cur_length, sums, dtype):
    """One transition as RolloutStorage.add_transitions + PPO.act / process_env_step + the runner's statistics leave it.  ``std``,
    ``time_outs`` and ``cur_return`` (with ``cur_length`` / ``sums``) may be None.  -> dict; ``terms`` = the returns added to sums[0]."""
    out = dict(obs=obs.clone(), actions=actions.clone(), mu=mean.clone(), rewards=rewards.clone(), dones=dones.clone(),
               time_outs=(time_outs != 0).float() if time_outs is not None else torch.zeros_like(rewards))
    if std is not None:
        out["sigma"] = std.expand_as(mean).clone()                     # mean * 0 + std
        out["log_prob"] = log_prob(actions, mean, std, dtype)
    if cur_return is not None:
        cr, cl, er, el = episode_step(cur_return, cur_length, rewards, dones, dtype)
        s = sums.to(dtype) + torch.stack((er.sum(), el.sum(), torch.tensor(float(er.numel()), dtype=dtype, device=er.device)))
        out.update(cur_return=cr, cur_length=cl, sums=s, terms=er)
    return out


def finish(actions, mean, rewards, dones, time_outs, std, cur_return, cur_length, sums, dtype):
    """The same bookkeeping for a segment already in the storage: [T, N, A] actions / mean, [T, N] rewards / dones / time_outs; every env's
    T steps are walked in order."""
    out = dict(sigma=std.expand_as(mean).clone(), log_prob=log_prob(actions, mean, std, dtype),
               time_outs=(time_outs != 0).float() if time_outs is not None else torch.zeros_like(rewards))
    if cur_return is not None:
        cr, cl, s, terms = cur_return.to(dtype), cur_length.to(dtype), sums.to(dtype), []
        for t in range(actions.shape[0]):
            cr, cl, er, el = episode_step(cr, cl, rewards[t], dones[t], dtype)
            s = s + torch.stack((er.sum(), el.sum(), torch.tensor(float(er.numel()), dtype=dtype, device=er.device)))
            terms.append(er)
        out.update(cur_return=cr, cur_length=cl, sums=s, terms=torch.cat(terms))
    return out


SUMS0 = (5.5, 40.0, 3.0)                  # the statistics do not start at zero
RECORD_STEPS = 3
RECORD_CASES = [(1, 3, 2), (17, 3, 3), (33, 16, 4), (257, 19, 6), (130, 235, 12), (50, 20, 16)]          # (N, observations, actions)
# form -> (std, time_outs given, storage_time_outs given, statistics)
RECORD_FORMS = {"legged": (True, True, True, True), "game": (False, False, False, True), "dec_agent": (False, True, True, True),
                "no_statistics": (True, True, True, False), "no_time_outs_in": (True, False, True, True)}
FINISH_CASES = [(1, 1, 2), (3, 5, 3), (24, 33, 12), (7, 257, 16), (24, 200, 12)]                        # (T, N, A); the last is a multiple of 256
# variant -> (time_outs given, time_outs_f given, statistics)
FINISH_VARIANTS = {"full": (True, True, True), "no_time_outs_in": (False, True, True), "no_time_outs_out": (True, False, True),
                   "no_statistics": (True, True, False)}


def policy_std(A, generator):
    """Policy std with an entry exactly 1.0, one at 0.05 and (from three actions) one at 3.0."""
    std = 0.5 + torch.rand(A, generator=generator)
    std[0], std[1] = 1.0, 0.05
    if A >= 3:
        std[2] = 3.0
    return std


def transitions(T, N, O, A, seed, p_done, forced):
    """Seeded CPU transitions [T, ...]: actions sampled as mean + std * eps; dones at ``p_done`` with the patterns of ``forced`` (a list of
    (env, [steps done])) written over them; half of the dones are time-outs."""
    g = torch.Generator().manual_seed(seed)
    std = policy_std(A, g)
    obs = torch.randn(T, N, O, generator=g) if O else None
    mean = torch.randn(T, N, A, generator=g) * 0.5
    actions = mean + std * torch.randn(T, N, A, generator=g)
    rewards = torch.randn(T, N, generator=g)
    dones = (torch.rand(T, N, generator=g) < p_done).to(torch.uint8)
    for env, steps in forced:
        if env < N:
            dones[:, env] = 0
            for t in steps:
                dones[t, env] = 1
    time_outs = ((dones != 0) & (torch.rand(T, N, generator=g) < 0.5)).to(torch.uint8)
    return dict(std=std, obs=obs, mean=mean, actions=actions, rewards=rewards, dones=dones, time_outs=time_outs,
                cur_return=torch.randn(N, generator=g), cur_length=torch.randint(0, 30, (N,), generator=g).float(), sums=torch.tensor(SUMS0))


def record_inputs(case):
    """Env 0 is done on steps 0 and 1 (consecutive), env 1 never; the others at 20 %."""
    N, O, A = case
    return transitions(RECORD_STEPS, N, O, A, seed=300 + N, p_done=0.2, forced=[(0, [0, 1]), (1, [])])


def assert_record_inputs(case, inp):
    N, O, A = case
    std, d = inp["std"], inp["dones"]
    assert bool((std == 1.0).any()) and bool((std == 0.05).any()) and (A < 3 or bool((std == 3.0).any()))
    assert tuple(float(x) for x in inp["sums"]) == SUMS0 and all(x != 0 for x in SUMS0)
    assert bool(((d[:-1] != 0) & (d[1:] != 0)).any()), "no env is done on consecutive steps"
    if N >= 17:
        assert 0.1 <= float(d.float().mean()) <= 0.3, float(d.float().mean())
    assert (N < 17 or bool(inp["time_outs"].any())) and not bool((inp["time_outs"] != 0)[d == 0].any())


def finish_inputs(case):
    """Two consecutive segments of T steps as one [2 T, ...] set.  Env 0 has no done; env 1 is done on the last step of the first segment
    (N = 1: env 0 is); env 2 (from T >= 3) has three dones in the first segment."""
    T, N, A = case
    forced = [(0, [T - 1])] if N == 1 else [(0, []), (1, [T - 1]), (2, [0, T // 2, T - 1] if T >= 3 else [])]
    return transitions(2 * T, N, 0, A, seed=500 + 11 * T + N, p_done=0.1, forced=forced)


def assert_finish_inputs(case, inp):
    T, N, A = case
    d = inp["dones"]
    first, second = d[:T].sum(0), d[T:].sum(0)
    assert bool((d[T - 1] != 0).any()), "no env is done on the last step of the first segment"
    if N >= 3:
        assert bool(((first == 0) & (second == 0)).any()), "no env without a done"
    if N >= 3 and T >= 3:
        assert bool((first >= 3).any() or (second >= 3).any()), "no env with three dones in one segment"
    assert (T * N * 16) % 256 != 0 or case == FINISH_CASES[-1]
    assert (FINISH_CASES[-1][0] * FINISH_CASES[-1][1] * 16) % 256 == 0
