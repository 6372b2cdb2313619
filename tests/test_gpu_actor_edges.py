"""The nine stand-alone MLP actor kernels behind ``lg_policy_act`` (csrc/lg_policy.h: k_policy_act<3,8,4,2>, k_policy_act<15|11|2|1,32,16,8>,
k_policy_act_wide<15|11|2|1,16,8,4>) and the two pack kernels that feed them, at their edges: the case table, the float64 reference,
the bars and their controls are tests/actor_check.py (tested on the CPU by tests/test_actor_check.py).  The entry points are called
directly through ``capi``; ``FusedActor`` where the wrapper is the subject (the device repack).

Every launch reads its observations from a window of a NaN-filled buffer and writes into NaN-filled outputs with ``EXTRA`` rows behind
row N: whatever the kernel leaves alone is still NaN afterwards, and a NaN row read for a live env makes its means NaN.  The exploration
noise is compared with ``tests/philox_np.action_noise`` (tests/noise_check.py).

Observed on an MI355X over the 98 cases: the exact kernels within 0.063 of their bar (float32 torch on the CPU: 0.033 at most), the
split-bf16 kernels within 0.23 of theirs (the float64 model of their arithmetic: 0.21), weights x 3 and observations x 100 included."""
import ctypes as C
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import actor_check as ac
from tests.noise_check import check_noise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EXTRA = 5                    # NaN rows behind row N of obs, actions and mean
LEAD = 2                     # NaN rows in front of the observation window
NAN = float("nan")


def _lib():
    from legged_games_gym_amd import capi
    return capi.load_library()


class _precision:
    """``lg_mlp_wide_set_precision(mode)`` for the block (None: left alone); the old value is put back on the way out."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.old = _lib().lg_mlp_wide_set_precision(self.mode) if self.mode is not None else None

    def __exit__(self, *exc):
        if self.mode is not None:
            _lib().lg_mlp_wide_set_precision(self.old)


def _linears(net):
    return [m for m in net if isinstance(m, nn.Linear)]


def _create(dims, net, std):
    """Raw ``lg_policy_create`` from host arrays (the host pack of the f32 layout; a 512-256-128 handle packs its split-bf16 operands on the
    device as well).  Returns (rc, handle)."""
    PF = C.POINTER(C.c_float)
    ws = [np.ascontiguousarray(m.weight.detach().float().cpu().numpy()) for m in _linears(net)]
    bs = [np.ascontiguousarray(m.bias.detach().float().cpu().numpy()) for m in _linears(net)]
    sd = np.ascontiguousarray(std.detach().float().cpu().numpy())
    handle = C.c_void_p()
    rc = _lib().lg_policy_create((C.c_int32 * 5)(*dims), (PF * 4)(*[w.ctypes.data_as(PF) for w in ws]), (PF * 4)(*[b.ctypes.data_as(PF) for b in bs]),
                                 sd.ctypes.data_as(PF), 0, C.byref(handle))
    return rc, handle


class _Actor:
    """A handle of ``lg_policy_create`` for an ``nn.Sequential`` on the CPU; ``with`` destroys it."""

    def __init__(self, net, std):
        lin = _linears(net)
        self.dims = [lin[0].in_features] + [m.out_features for m in lin]
        rc, self.handle = _create(self.dims, net, std)
        assert rc == 0, (rc, _lib().lg_last_error().decode())

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        _lib().lg_policy_destroy(self.handle)
        self.handle = None

    def load_device(self, net_dev, std_dev):
        """Raw ``lg_policy_load_device`` from parameters on the device (the device pack of both layouts)."""
        lin = _linears(net_dev)
        ptr = C.c_void_p * 4
        rc = _lib().lg_policy_load_device(self.handle, ptr(*[m.weight.data_ptr() for m in lin]), ptr(*[m.bias.data_ptr() for m in lin]),
                                          std_dev.data_ptr(), torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
        assert rc == 0, (rc, _lib().lg_last_error().decode())

    def act(self, obs, N, seed=5, step=3, counter=None, deterministic=False, with_mean=True, expect=0):
        """One raw ``lg_policy_act`` on rows 0 .. N - 1 of ``obs``; returns the FULL ``actions`` / ``mean`` buffers ([N + EXTRA, actions], NaN
        where nothing was written)."""
        nA = self.dims[4]
        actions = torch.full((N + EXTRA, nA), NAN, device=DEV)
        mean = torch.full((N + EXTRA, nA), NAN, device=DEV)
        rc = _lib().lg_policy_act(self.handle, obs.data_ptr(), actions.data_ptr(), mean.data_ptr() if with_mean else None, N, seed, step,
                                  counter.data_ptr() if counter is not None else None, int(deterministic),
                                  torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
        torch.cuda.synchronize()
        assert rc == expect, (rc, _lib().lg_last_error().decode())
        return actions, mean


def _window(obs):
    """``obs`` [N, width] on the device as a contiguous window of a NaN-filled buffer: LEAD NaN rows before it, EXTRA behind it."""
    n, width = obs.shape
    full = torch.full((LEAD + n + EXTRA, width), NAN, device=DEV)
    full[LEAD:LEAD + n] = obs.to(DEV)
    view = full[LEAD:LEAD + n]
    assert view.is_contiguous() and bool(torch.isnan(full[:LEAD]).all()) and bool(torch.isnan(full[LEAD + n:]).all())
    return view


def _assert_rows(label, got, want, bar, N, wg_envs=None):
    """Every element of rows 0 .. N - 1 finite and within ``bar`` of ``want`` (float64, CPU), every element behind row N still NaN.  With
    ``wg_envs`` a miss names the worst error of each workgroup, so that a wrong rotation of the weight stream names its block."""
    g = got.detach().double().cpu()
    assert bool(torch.isnan(g[N:]).all()), f"{label}: {int((~torch.isnan(g[N:])).sum())} guard elements behind row {N} were written"
    assert bool(torch.isfinite(g[:N]).all()), f"{label}: {int((~torch.isfinite(g[:N])).sum())} elements of the first {N} rows are not finite"
    err = (g[:N] - want).abs()
    worst = float(err.max())
    if not worst < bar and wg_envs:
        per_wg = [f"wg {b} (r1 {(5 * b) % ac.ROTATIONS}, share {b % 8}): {float(err[b * wg_envs:(b + 1) * wg_envs].max()) / bar:.2f}"
                  for b in range((N + wg_envs - 1) // wg_envs)]
        raise AssertionError(f"{label}: max error {worst:.3e} >= {bar:.3e}; bars per workgroup: " + ", ".join(per_wg))
    assert worst < bar, f"{label}: max error {worst:.3e} >= {bar:.3e} at {np.unravel_index(int(err.argmax()), err.shape)}"
    return worst


def _guards_untouched(*bufs):
    return all(bool(torch.isnan(b).all()) for b in bufs)


@pytest.mark.parametrize("cid", ac.CASE_IDS)
def test_means_match_float64_with_guard_rows_intact(cid):
    """Every row of ``actor_check.CASES``: the means of a host-created handle against float64 within the kernel's bar, the sampled actions
    finite, nothing written behind row N; then the same parameters packed on the device (``lg_policy_load_device``) give the same bits."""
    r = ac.reference(cid)
    c, k = r.case, r.case.kernel
    N = c.num_envs
    obs = _window(r.obs)
    with _precision(k.precision), _Actor(r.net, r.std) as actor:
        actions, mean = actor.act(obs, N)
        try:
            err = _assert_rows(f"{cid} mean", mean, r.want, r.bar, N, k.wg_envs if k.build == "wide" and N > 33 else None)
        finally:
            e = (mean[:N].double().cpu() - r.want).abs()
            print(f"[observed] actor {cid}: mean err {float(e.max()):.3e} = {float(e.max()) / r.bar:.3f} of the bar {r.bar:.3e} (scale {r.scale:.3f}); "
                  f"{'float32 torch' if k.build == 'exact' else 'split-bf16 model'} on the CPU {r.control / r.bar:.3f}")
        assert bool(torch.isfinite(actions[:N]).all()) and bool(torch.isnan(actions[N:]).all())
        assert float((actions[:N] - mean[:N]).abs().max()) > 0.0                     # (the noise itself: the test below)
        dev_net, dev_std = ac.wl.float64_copy(r.net).float().to(DEV), r.std.to(DEV)
        actor.load_device(dev_net, dev_std)
        a2, m2 = actor.act(obs, N)
        assert torch.equal(m2[:N], mean[:N]) and torch.equal(a2[:N], actions[:N]), f"{cid}: the device pack differs from the host pack"
        assert bool(torch.isnan(a2[N:]).all()) and bool(torch.isnan(m2[N:]).all())
    assert err < r.bar


# one ragged case per kernel: 13 actions (a last lane group of one), one env past a workgroup
FLAG_CASES = [c.id for c in ac.CASES if c.num_actions == 13 and c.num_envs == c.kernel.wg_envs + 1]


@pytest.mark.parametrize("cid", FLAG_CASES)
def test_flags_at_a_ragged_case(cid):
    r = ac.reference(cid)
    k, N = r.case.kernel, r.case.num_envs
    obs = _window(r.obs)
    seed, step = 5, 3
    with _precision(k.precision), _Actor(r.net, r.std) as actor:
        actions, mean = actor.act(obs, N, seed, step)
        _assert_rows(f"{cid} mean", mean, r.want, r.bar, N)
        det_a, det_m = actor.act(obs, N, seed, step, deterministic=True)             # deterministic: actions ARE the means
        assert torch.equal(det_a[:N], det_m[:N]) and torch.equal(det_m[:N], mean[:N]) and _guards_untouched(det_a[N:], det_m[N:])
        no_a, no_m = actor.act(obs, N, seed, step, with_mean=False)                  # mean = NULL: the same actions, no mean
        assert torch.equal(no_a[:N], actions[:N]) and _guards_untouched(no_a[N:], no_m)
        again_a, again_m = actor.act(obs, N, seed, step)                             # the same (seed, step): the same bits
        assert torch.equal(again_a[:N], actions[:N]) and torch.equal(again_m[:N], mean[:N])
        other_a, other_m = actor.act(obs, N, seed, step + 1)                         # another step: other noise on the same means
        assert torch.equal(other_m[:N], mean[:N]) and _guards_untouched(other_a[N:], other_m[N:])
        assert float(((other_a[:N] - other_m[:N]) - (actions[:N] - mean[:N])).abs().mean()) > 0.1      # two independent draws of std >= 0.3
        for n in (1, k.wg_envs):                                                     # rows are independent of how many there are
            a, m = actor.act(obs, n, seed, step)
            assert torch.equal(a[:n], actions[:n]) and torch.equal(m[:n], mean[:n]) and _guards_untouched(a[n:], m[n:]), n
    assert len(FLAG_CASES) == len(ac.KERNELS)


@pytest.mark.parametrize("nA", [1, 5, 12, 13, 16])
def test_noise_is_the_reference_stream_for_every_action_count(nA):
    """``actions - mean`` is ``std * eps`` of the NumPy Philox reference for (seed; env, step), from the exact and from the split-bf16
    kernel of the 19-observation shape, with the step given by value and taken from a device counter holding step - 1 (left alone); the
    two builds draw the same samples.  37 envs: three workgroups of 16 or two of 32, the last one ragged."""
    N, seed, step = 37, 9, 41
    net, obs_cpu, std = ac.make_inputs(19, ac.WIDE_HIDDEN, nA, N, "default", 500 + nA)
    assert nA == 1 or float(std.diff().min()) > 0.0
    obs, std64, report, noise = _window(obs_cpu), std.double().numpy(), {}, []
    for precision in (0, 1):
        assert ac.kernel_for(ac.WIDE_HIDDEN, 19, precision) == ("exact2", "wide2")[precision]
        with _precision(precision), _Actor(net, std) as actor:
            actions, mean = actor.act(obs, N, seed, step)
            check_noise(actions[:N].cpu().numpy(), mean[:N].cpu().numpy(), std64, seed, step, report)
            assert _guards_untouched(actions[N:], mean[N:])
            counter = torch.tensor([step - 1], dtype=torch.int64, device=DEV)
            by_counter, m_counter = actor.act(obs, N, seed, -1, counter=counter)
            assert int(counter[0]) == step - 1
            assert torch.equal(by_counter[:N], actions[:N]) and torch.equal(m_counter[:N], mean[:N]) and _guards_untouched(by_counter[N:], m_counter[N:])
            counter += 7
            later, m_later = actor.act(obs, N, seed, -1, counter=counter)
            check_noise(later[:N].cpu().numpy(), m_later[:N].cpu().numpy(), std64, seed, step + 7, report)
            assert torch.equal(m_later[:N], mean[:N])
            noise.append((actions[:N].double().cpu().numpy(), mean[:N].double().cpu().numpy()))
    (a0, m0), (a1, m1) = noise
    diff = np.abs((a1 - m1) - (a0 - m0))
    assert (diff <= 1e-6 * (1.0 + np.abs(a0) + np.abs(a1))).all(), float(diff.max())      # float32 roundings of mean + noise on two means
    print(f"[observed] actor noise nA={nA}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(report.items())) + f", exact vs split {float(diff.max()):.3g}")


@pytest.mark.parametrize("name,width", [(k.name, w) for k, w in ac.REPACK])
def test_device_repack_equals_host_pack_at_the_padded_widths(name, width):
    """``FusedActor.sync_device()`` after every parameter and ``std`` moved, at the first and the last observation width of the kernel's
    range: within the bar of float64 on the NEW parameters, and bit-equal to a fresh ``FusedActor`` of the same module (host pack of the
    f32 layout, a first device pack of the split-bf16 one)."""
    from legged_games_gym_amd.rl import FusedActor
    k = next(x for x in ac.KERNELS if x.name == name)
    N, nA = k.wg_envs + 1, 13
    net, obs_cpu, std = ac.make_inputs(width, k.hidden, nA, N, "default", 700 + width)
    policy = types.SimpleNamespace(actor=net.to(DEV), std=std.to(DEV))
    obs = _window(obs_cpu)
    with _precision(k.precision):
        assert ac.kernel_for(k.hidden, width, 1 if k.precision is None else k.precision) == name
        first = FusedActor(policy, DEV, seed=5)
        _, before = (t.clone() for t in first.act_with_mean(obs))
        g = torch.Generator().manual_seed(width)
        with torch.no_grad():
            for prm in policy.actor.parameters():
                prm.add_((0.05 * torch.randn(prm.shape, generator=g)).to(DEV))
            policy.std.mul_(0.7)
        first.sync_device()
        a_first, m_first = (t.clone() for t in first.act_with_mean(obs))
        fresh = FusedActor(policy, DEV, seed=5)
        fresh._host_step = first._host_step - 1                                      # the same Philox step as the call above
        a_fresh, m_fresh = (t.clone() for t in fresh.act_with_mean(obs))
        torch.cuda.synchronize()
    assert a_first.shape == (N, nA) and torch.equal(m_first, m_fresh) and torch.equal(a_first, a_fresh)
    assert not torch.equal(m_first, before)
    want = ac.float64_forward(policy.actor.cpu(), obs_cpu, f"{name} {width}")
    scale = max(1.0, float(want.abs().max()))
    err = ac.max_err(m_first, want)
    print(f"[observed] actor repack {name} obs{width}: mean err {err:.3e} = {err / (ac.tol(k) * scale):.3f} of the bar (scale {scale:.3f})")
    assert bool(torch.isfinite(m_first).all()) and err < ac.tol(k) * scale
    check_noise(a_first.cpu().numpy(), m_first.cpu().numpy(), policy.std.double().cpu().numpy(), 5, first._host_step, {})      # the new std arrived


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("hidden,width", ac.REFUSED_AT_ACT, ids=[f"{h[0]}-{o}" for h, o in ac.REFUSED_AT_ACT])
def test_unserved_widths_are_refused_and_nothing_is_launched(hidden, width, precision):
    N = 17
    net, obs_cpu, std = ac.make_inputs(width, hidden, 12, N, "default", width)
    obs = _window(obs_cpu)
    with _precision(precision), _Actor(net, std) as actor:                           # creation accepts the shape: the refusal is the dispatch's
        actions, mean = actor.act(obs, N, expect=-4)
        assert _guards_untouched(actions, mean)
        assert b"compiled-in shapes" in _lib().lg_last_error()


def test_create_refuses_what_no_kernel_can_hold_and_zero_envs_write_nothing():
    for dims in ac.REFUSED_AT_CREATE:
        net = ac.wl.make_mlp(dims[0], dims[1:4], dims[4], 1)
        rc, handle = _create(dims, net, torch.ones(dims[4]))
        assert rc == -4 and not handle, (dims, rc)
    r = ac.reference(ac.CASE_IDS[0])
    with _Actor(r.net, r.std) as actor:
        actions, mean = actor.act(_window(r.obs), 0)
        assert _guards_untouched(actions, mean)
