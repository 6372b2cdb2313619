"""-m gpu: the LDS-resident learner kernels of the 48-128-64-32 tasks (csrc/lg_train.h: k_mlp_train forward / backward / backward with the
PPO loss inside, k_mlp_reduce) against float64 at their edges: the input and output widths at which the loads change path, the
mini-batch sizes at which the row-tile schedule and the partial-sum loop change path (tests/flat_learner_check.py derives them from the
device's compute-unit count), gathers with repeated rows, and the in-kernel loss on both sides of every clip edge.

Every reference is float64 autograd on deep copies of the same modules and .double() copies of the same tables, computed on the host
(so the references do not depend on the device); torch's own float32 autograd on the same modules is printed beside the kernel's error
and must itself stay within a quarter of the gradient bound, so the bound has room by construction.  Before every launch the outputs,
every .grad, d_std, stats and the WHOLE workspace are NaN: an element or a partial a workgroup does not write shows up as non-finite."""
import copy

import pytest
import torch

from tests import flat_learner_check as fl
from tests import wide_learner_check as wl

pytestmark = pytest.mark.gpu

D_STD_TOL = (1e-4, 1e-6)                       # of max + absolute: test_ppo_loss_kernel_matches_float64_at_the_games_action_counts
CLIP, VCOEF, ECOEF = 0.2, 1.0, 0.01


def _stats_tol(ref):
    return 2e-5 * max(1.0, float(ref.abs().max()))


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count          # the attribute mlp_fill reads


def _assert_schedule(c, cus):
    """The case is the edge it is listed for: mlp_fill (restated) launches what the derivation says."""
    slots, partials = fl.BUILDS[c.build]
    assert fl.schedule(c.mb, c.n_nets, slots, partials, cus) == (c.n_tiles, c.wgs, c.n_iter, c.idle), (c, cus)


# ---- forward / backward from a given dL/dy ------------------------------------------------------------------------------------

def _problem(spec, shared, mb, table_rows, seed, scale=2.0):
    """Host side of a case: the networks (float32, torch's default initialisation), their input tables (randn * scale: both ELU branches
    in every layer) and dL/dy; table_rows > mb means the mini-batch is gathered."""
    nets = [wl.make_mlp(i, fl.HIDDEN, o, 10 * seed + n) for n, (i, o) in enumerate(spec)]
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(table_rows, spec[0][0], generator=g) * scale]
    for i, _ in spec[1:]:
        xs.append(xs[0] if shared else torch.randn(table_rows, i, generator=g) * scale)
    d_out = [torch.randn(mb, o, generator=g) / mb for _, o in spec]
    return nets, xs, d_out, g


def _reference(nets, xs, rows, mb, d_out, backward=True):
    """float64 outputs and parameter gradients, and the error of torch's float32 pass on the same modules against them.  The float32
    gradients must be within a quarter of the kernels' bound: the inputs are well-conditioned."""
    refs = [wl.float64_copy(n) for n in nets]
    xb = [(x[rows] if rows is not None else x[:mb]) for x in xs]
    for n, (r, x) in enumerate(zip(refs, xb)):
        if mb >= 32:                                               # a share of a handful of rows says nothing
            wl.assert_both_elu_branches(r, x.double(), f"net {n}")
    want_out = [r(x.double()) for r, x in zip(refs, xb)]
    f32_out = [n(x) for n, x in zip(nets, xb)]
    f32_err = [wl.max_error(f32_out, want_out, False), float("nan")]
    want = []
    if backward:
        torch.autograd.backward(want_out, [d.double() for d in d_out])
        torch.autograd.backward(f32_out, d_out)
        want = [p.grad.clone() for r in refs for p in r.parameters()]
        f32_grads = [p.grad.clone() for n in nets for p in n.parameters()]
        f32_err[1] = wl.compare_all(["float32 torch " + l for l in wl.param_labels(nets)], f32_grads, want, rel=wl.GRAD_TOL[0] / 4, abs_tol=wl.GRAD_ABS / 4)
    return [w.detach() for w in want_out], want, f32_err


def _device_nets(nets):
    """Copies of the networks on the device, every .grad NaN."""
    dev = [copy.deepcopy(n).cuda() for n in nets]
    for net in dev:
        for p in net.parameters():
            p.grad = torch.full_like(p, float("nan"))
    return dev


def _trainer(nets, xs, mb):
    from legged_games_gym_amd.rl.mlp_kernels import MlpTrainer
    dev = _device_nets(nets)
    dxs = [x.cuda() for x in xs]
    if len(xs) > 1 and xs[1] is xs[0]:
        dxs[1] = dxs[0]
    tr = MlpTrainer(dev, dxs, mb)
    assert tr.supported
    return tr, dev


def _nan_fill(tr, dev):
    for o in tr.outputs:
        o.fill_(float("nan"))
    for net in dev:
        for p in net.parameters():
            p.grad.fill_(float("nan"))
    tr.workspace.fill_(float("nan"))                               # it comes from torch.empty; k_mlp_reduce sums every launched partial


def _launch(tr, dev, rows, d_out, forward=True, backward=True):
    """NaN everywhere, then lg_mlp_forward and / or lg_mlp_backward; clones of the outputs and of every parameter gradient."""
    _nan_fill(tr, dev)
    outs = [o.clone() for o in tr.forward(rows)] if forward else []
    grads = []
    if backward:
        for buf, d in zip(tr.grad_outputs, d_out):
            buf.copy_(d)
        tr.backward(rows)
        grads = [p.grad.clone() for n in dev for p in n.parameters()]
    torch.cuda.synchronize()
    return outs, grads


def _check(label, nets, got, want, f32_err):
    (outs, grads), (want_out, want_grads) = got, want
    fig = []
    if outs:
        fig.append(f"outputs {wl.max_error([o.cpu() for o in outs], want_out, False):.3g} (torch f32 {f32_err[0]:.3g})")
    if grads:
        fig.append(f"gradients {wl.max_error([h.cpu() for h in grads], want_grads, True):.3g} of max (torch f32 {f32_err[1]:.3g})")
    print(f"[observed] flat {label}: " + ", ".join(fig))
    if outs:
        wl.compare_all([f"net{n}.output" for n in range(len(nets))], outs, want_out, abs_tol=wl.OUT_TOL[0])
    if grads:
        wl.compare_all(wl.param_labels(nets), grads, want_grads, rel=wl.GRAD_TOL[0], abs_tol=wl.GRAD_ABS)


def _forward_backward_case(label, spec, shared, mb, table_rows, seed, rows=None, forward=True, backward=True):
    nets, xs, d_out, g = _problem(spec, shared, mb, table_rows, seed)
    if rows is None and table_rows > mb:
        rows = torch.randperm(table_rows, generator=g)[:mb]
    want_out, want_grads, f32_err = _reference(nets, xs, rows, mb, d_out, backward)
    tr, dev = _trainer(nets, xs, mb)
    drows = rows.cuda() if rows is not None else None
    dd = [d.cuda() for d in d_out]
    got = _launch(tr, dev, drows, dd, forward, backward)
    _check(label, nets, got, (want_out, want_grads), f32_err)
    again = _launch(tr, dev, drows, dd, forward, backward)           # fixed reduction order: bit-reproducible
    assert all(torch.equal(a, b) for a, b in zip(got[0] + got[1], again[0] + again[1]))
    return nets, xs, d_out, rows, got


# actor widths against output widths, each table in both directions, the critic on the actor's table; the critic pairings; one single net
_WIDTHS = [pytest.param([(i, o), (i, 1)], True, id=f"{i}-{o}_and_{i}-1") for i, o in zip(fl.ACTOR_INPUTS, fl.OUTPUTS)] + \
          [pytest.param([(i, o), (i, 1)], True, id=f"{i}-{o}_and_{i}-1") for i, o in zip(fl.ACTOR_INPUTS, reversed(fl.OUTPUTS))] + \
          [pytest.param([(a, 12), (c, 1)], False, id=f"sep_{a}-12_and_{c}-1") for a, c in fl.CRITIC_PAIRS] + \
          [pytest.param([(17, 5)], False, id="single_17-5")]


@pytest.mark.parametrize("mb,gather", wl.MB_SMALL)
@pytest.mark.parametrize("spec,shared", _WIDTHS)
def test_forward_and_backward_match_float64_over_widths(spec, shared, mb, gather):
    """lg_mlp_forward / lg_mlp_backward over flat_learner_check's width tables (scalar, mixed and vector paths of LdsFill::load and
    request(), waves with no live input column, 1 .. 16 outputs), two nets on one table, two nets on separate tables of different widths
    and a single net, at 37 rows (no gather) and 516 gathered rows.  Outputs 2e-5 absolute, gradients 1e-4 of each tensor's max + 1e-10.
    [observed] on an MI355X: outputs <= 3.1e-07 (torch f32 <= 3.6e-07), gradients <= 4.9e-06 of max (torch f32 <= 2.8e-06)."""
    assert not any(i > 48 or o > 16 for i, o in spec)
    label = f"{[(i, *fl.HIDDEN, o) for i, o in spec]} mb {mb}"
    _forward_backward_case(label, spec, shared, mb, 3000 if gather else mb, seed=3)


def test_another_hidden_shape_is_refused():
    """mlp_fill builds 128-64-32 only: anything else is reported, not mis-computed."""
    from legged_games_gym_amd.rl.mlp_kernels import MlpTrainer
    wide = wl.make_mlp(48, wl.GAME_HIDDEN, 12, 0).cuda()
    assert not MlpTrainer([wide], [torch.randn(64, 48, device="cuda")], 64).supported
    odd = wl.make_mlp(48, (128, 64, 16), 12, 0).cuda()
    assert not MlpTrainer([odd], [torch.randn(64, 48, device="cuda")], 64).supported


_SCHEDULE = [pytest.param(build, cid, id=cid) for build in ("forward", "backward") for cid in fl.CASE_IDS[build]]


@pytest.mark.parametrize("build,cid", _SCHEDULE)
def test_forward_and_backward_match_float64_over_the_schedule(build, cid):
    """48 -> 12 and 48 -> 1 (n_nets = 1: 48 -> 12 alone), gathered, at every flat_learner_check.mb_cases entry for this device's
    compute-unit count: one tile of 1 / 15 / 16 rows, a wholly idle 4-wave group, 1 .. 25 partials for k_mlp_reduce, a second and a
    third trip of the persistent loop with one live group.  A forward case runs lg_mlp_forward, a backward case lg_mlp_backward.
    [observed] on an MI355X (256 CUs): outputs <= 2.5e-07 (torch f32 <= 2.5e-07), gradients <= 1.8e-06 of max (torch f32 <= 3.0e-06)."""
    cus = _cus()
    c = fl.case(cus, cid)
    assert c.build == build
    _assert_schedule(c, cus)
    spec = [(48, 12), (48, 1)][:c.n_nets]
    _forward_backward_case(f"{cid} ({cus} CUs) mb {c.mb} tiles {c.n_tiles} wgs {c.wgs} trips {c.n_iter} idle groups {c.idle}", spec, True, c.mb,
                           c.mb + 200, seed=7, forward=build == "forward", backward=build == "backward")


@pytest.mark.parametrize("d0", [47, 48])
def test_gather_with_duplicates_and_table_ends(d0):
    """A row list in which a third of the indices repeat others and which holds the first and the last table row (dW must count both
    copies), scalar (47) and vector (48) gather; then the same mini-batch with rows = None on a table that IS the gathered copy: the
    arithmetic is the same, so outputs and gradients are bit-identical.
    [observed] on an MI355X: outputs <= 1.9e-07 (torch f32 <= 2.0e-07), gradients <= 7.0e-07 of max (torch f32 <= 5.1e-07); the two
    launches agree bit for bit."""
    mb, R = 16 * 9 + 5, 400
    rows = fl.rows_with_duplicates(torch.Generator().manual_seed(d0), mb, R)
    assert rows.numel() == mb and rows.unique().numel() <= mb - mb // 3 and int(rows.min()) == 0 and int(rows.max()) == R - 1
    spec = [(d0, 12), (d0, 1)]
    nets, xs, d_out, _, got = _forward_backward_case(f"duplicate rows {d0}", spec, True, mb, R, seed=11, rows=rows)
    tr, dev = _trainer(nets, [xs[0][rows].contiguous()] * 2, mb)
    direct = _launch(tr, dev, None, [d.cuda() for d in d_out])
    assert all(torch.equal(a, b) for a, b in zip(got[0] + got[1], direct[0] + direct[1]))


# ---- forward + PPO loss + backward in one kernel (lg_ppo_minibatch) ------------------------------------------------------------

def _fused_problem(A, mb, table_rows, seed, far=False, scale=2.0):
    """Host side of a fused case: actor 48 -> A, critic 48 -> 1 on one observation table, a storage-like loss table with old_sigma per
    action and different from std, old_log_prob / old values placed from the FLOAT64 forward of the two networks so that ratios and value
    steps lie on both sides of the clip edges, 5 % of the rows with an advantage of exactly 0 (t1 == t2: the reference's gradient is 0).
    far: a sixteenth of the rows get log ratio uniform in +-[5, 15]."""
    nets = [wl.make_mlp(48, fl.HIDDEN, A, 10 * seed), wl.make_mlp(48, fl.HIDDEN, 1, 10 * seed + 1)]
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(table_rows, 48, generator=g) * scale
    ix = torch.randperm(table_rows, generator=g)[:mb]
    std = 0.5 + 1.0 * torch.rand(A, generator=g)
    t = wl.loss_tables(A, table_rows, g, dev="cpu")
    assert float((std - t["old_sigma"][0]).abs().min()) > 1e-3 and float(t["old_sigma"][0].std() if A > 1 else 1.0) > 0.0
    xb = obs[ix].double()
    with torch.no_grad():
        mu64, val64 = (wl.float64_copy(n)(xb) for n in nets)
    wl.place_ratios_and_value_steps(t, ix, mu64, std, val64, g, CLIP)
    n_zero = (mb + 19) // 20
    t["adv"][ix[:n_zero]] = 0.0
    if far:
        n_far = mb // 16
        far_rows = ix[n_zero:n_zero + n_far]
        lp = torch.distributions.Normal(mu64, mu64 * 0.0 + std.double()).log_prob(t["actions"][ix].double()).sum(-1)[n_zero:n_zero + n_far]
        sign = torch.where(torch.arange(n_far) % 2 == 0, 1.0, -1.0).double()
        log_ratio = sign * (5.0 + 10.0 * torch.rand(n_far, generator=g, dtype=torch.float64))
        t["old_lp"][far_rows, 0] = (lp - log_ratio).float()
        a = t["adv"][far_rows, 0].abs().clamp_min(0.1) * torch.where((torch.arange(n_far) // 2) % 2 == 0, 1.0, -1.0)
        t["adv"][far_rows, 0] = a
        for s in (1.0, -1.0):                                      # both signs of advantage on both sides
            assert bool(((a > 0) & (sign == s)).any()) and bool(((a < 0) & (sign == s)).any())
    return nets, obs, ix, std, t


def _fused_reference(nets, obs, ix, std, t, clipped, dtype, margin_only):
    """Loss statistics and every gradient of surrogate + vc * value loss - ec * entropy by autograd in ``dtype``, observations to parameters."""
    mods = [wl.float64_copy(n) if dtype == torch.float64 else copy.deepcopy(n) for n in nets]
    s_ = std.to(dtype).requires_grad_()
    xb = obs[ix].to(dtype)
    mu, val = mods[0](xb), mods[1](xb)
    s, v, kl, ent, ratio, dv = wl.ppo_loss(mu, s_, val, *(t[k][ix].to(dtype) for k in ("actions", "old_lp", "old_mu", "old_sigma", "adv", "old_val", "ret")), CLIP, clipped)
    if dtype == torch.float64:
        if ix.numel() >= 64:
            wl.assert_both_elu_branches(mods[0], xb, "actor"); wl.assert_both_elu_branches(mods[1], xb, "critic")
        wl.assert_loss_inputs_not_degenerate(ratio, dv, CLIP, share=0.0 if margin_only else 0.20, margin=1e-2)
    (s + VCOEF * v - ECOEF * ent).backward()
    return torch.stack((s, v, kl, ent)).detach(), [p.grad for m in mods for p in m.parameters()], s_.grad


def _fused_launch(nets, obs, ix, std, t, clipped, loss_acc=None):
    """lg_ppo_minibatch through MlpTrainer.ppo_minibatch on NaN-filled gradients, d_std, stats and workspace."""
    from legged_games_gym_amd import capi
    A, mb = std.numel(), ix.numel()
    dobs = obs.cuda()
    tr, dev = _trainer(nets, [dobs, dobs], mb)
    _nan_fill(tr, dev)
    dt = {k: v.cuda().contiguous() for k, v in t.items()}
    dix, dstd = ix.cuda(), std.cuda()
    d_std, stats = torch.full((A,), float("nan"), device="cuda"), torch.full((4,), float("nan"), device="cuda")
    p = lambda x: x.data_ptr()
    b = capi.lg_ppo_batch()
    b.actions, b.old_log_prob, b.old_mu, b.old_sigma = p(dt["actions"]), p(dt["old_lp"]), p(dt["old_mu"]), p(dt["old_sigma"])
    b.advantages, b.old_values, b.returns, b.std = p(dt["adv"]), p(dt["old_val"]), p(dt["ret"]), p(dstd)
    b.clip, b.value_coef, b.entropy_coef, b.use_clipped_value = CLIP, VCOEF, ECOEF, clipped
    b.d_std, b.stats = p(d_std), p(stats)
    acc = None
    if loss_acc is not None:
        acc = torch.tensor(loss_acc, device="cuda")
        b.loss_acc = p(acc)
    tr.ppo_minibatch(dix, b)
    torch.cuda.synchronize()
    return [q.grad.clone() for n in dev for q in n.parameters()], d_std, stats, acc


def _fused_case(label, A, mb, table_rows, clipped, seed, far=False, with_loss_acc=False):
    nets, obs, ix, std, t = _fused_problem(A, mb, table_rows, seed, far)
    ref, want, want_std = _fused_reference(nets, obs, ix, std, t, clipped, torch.float64, margin_only=mb < 64)
    f32_ref, f32_grads, f32_std = _fused_reference(nets, obs, ix, std, t, clipped, torch.float32, True)
    labels = wl.param_labels(nets)
    f32_err = (wl.max_error([f32_ref], [ref], False),
               wl.compare_all(["float32 torch " + l for l in labels], f32_grads, want, rel=wl.GRAD_TOL[0] / 4, abs_tol=wl.GRAD_ABS / 4),
               wl.compare("float32 torch d_std", f32_std, want_std, rel=D_STD_TOL[0] / 4, abs_tol=D_STD_TOL[1] / 4))
    grads, d_std, stats, _ = _fused_launch(nets, obs, ix, std, t, clipped)
    print(f"[observed] fused {label}: stats {wl.max_error([stats.cpu()], [ref], False):.3g} of {float(ref.abs().max()):.3g} (torch f32 {f32_err[0]:.3g}), "
          f"gradients {wl.max_error([h.cpu() for h in grads], want, True):.3g} of max (torch f32 {f32_err[1]:.3g}), "
          f"d_std {wl.max_error([d_std.cpu()], [want_std], True):.3g} of max (torch f32 {f32_err[2]:.3g})")
    wl.compare("stats", stats, ref, abs_tol=_stats_tol(ref))
    wl.compare_all(labels, grads, want, rel=wl.GRAD_TOL[0], abs_tol=wl.GRAD_ABS)
    wl.compare("d_std", d_std, want_std, rel=D_STD_TOL[0], abs_tol=D_STD_TOL[1])
    if with_loss_acc:                                              # the update's running sums: += {value-loss mean, surrogate mean}
        preset = (0.25, -0.5)
        grads2, d_std2, stats2, acc = _fused_launch(nets, obs, ix, std, t, clipped, loss_acc=preset)
        want_acc = torch.tensor(preset, dtype=torch.float64) + torch.stack((ref[1], ref[0]))
        wl.compare("loss_acc", acc, want_acc, abs_tol=_stats_tol(ref))
        assert torch.equal(stats, stats2) and torch.equal(d_std, d_std2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))


@pytest.mark.parametrize("clipped", [1, 0])
@pytest.mark.parametrize("A", fl.OUTPUTS)
def test_fused_minibatch_matches_float64_over_action_counts(A, clipped):
    """lg_ppo_minibatch (k_mlp_train<..., LOSS>) against float64 autograd of the WHOLE loss, observations to parameters, for 1 .. 16
    actions (lane groups of a row idle for A <= 12, quad() loads scalar for A & 3, none idle at 16), clipped and plain value loss,
    mb = 16 * 11 + 9 gathered from 600 rows: every parameter gradient of both nets (1e-4 of each tensor's max + 1e-10), d_std with the
    entropy term (1e-4 of max + 1e-6) and stats[0..3] (2e-5 * max(1, |ref|)); then a second launch whose loss_acc starts at
    (0.25, -0.5) and must end at that + (value-loss mean, surrogate mean).
    [observed] on an MI355X: stats <= 9.3e-07 (torch f32 <= 1.9e-06), gradients <= 4.0e-06 of max (torch f32 <= 5.7e-06), d_std <= 3.0e-05
    of max (torch f32 <= 1.6e-05)."""
    _fused_case(f"A {A} clipped {clipped}", A, 16 * 11 + 9, 600, clipped, seed=100 * A + clipped, with_loss_acc=True)


@pytest.mark.parametrize("cid", [c for c in fl.CASE_IDS["backward"] if c.startswith("backward2-")])
def test_fused_minibatch_matches_float64_over_the_schedule(cid):
    """A = 12 at every two-net backward-build entry of flat_learner_check.mb_cases (lg_ppo_minibatch takes actor and critic, so the
    single-net entries do not apply).  For mb < 64 the shares of rows inside / outside the clip ranges cannot hold (at mb = 1 there is
    one row): there only the distance of every row from a clip edge is asserted on the reference.
    [observed] on an MI355X (256 CUs): stats <= 2.2e-06 (torch f32 <= 8.5e-06), gradients <= 3.1e-06 of max (torch f32 <= 5.2e-06), d_std
    <= 2.4e-06 of max (torch f32 <= 6.9e-06)."""
    cus = _cus()
    c = fl.case(cus, cid)
    _assert_schedule(c, cus)
    _fused_case(f"{cid} ({cus} CUs) mb {c.mb} wgs {c.wgs} trips {c.n_iter} idle groups {c.idle}", 12, c.mb, c.mb + 200, 1, seed=13)


def test_fused_minibatch_far_outside_the_clip_range():
    """A = 12, mb = 200, a sixteenth of the rows with log ratio uniform in +-[5, 15] and both signs of advantage on either side (the
    others placed as above): __expf at large arguments, ratios of 1e-7 .. 3e6.  Everything finite, stats within 2e-5 * max(1, |ref|),
    gradients within the usual bound -- of a max that these rows dominate, which is why the ordinary rows have tests of their own.
    [observed] on an MI355X: stats 4.4e-04 of a surrogate of 7.9e+03 (torch f32 5.4e-05), gradients 6.3e-07 of max (torch f32 1.0e-06), d_std
    9.6e-08 of max (torch f32 3.0e-07)."""
    _fused_case("far outside", 12, 200, 600, 1, seed=17, far=True)
