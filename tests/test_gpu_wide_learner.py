"""-m gpu: the wide learner kernels (csrc/lg_gemm.h, lg_ppo_loss) against float64 at the shapes of the predator-prey tasks --
19 / 16 / 3 inputs, 512-256-128 hidden, 6 / 4 / 2 / 1 outputs -- which lg_mlp_wide_forward sends down the per-layer GEMM path
(k_wide_prep, k_gemm_wide[_bf16x3]<FWD>), never the chain kernel; plus the shapes around them where the kernels change path."""
import os

import pytest
import torch

from tests import wide_learner_check as wl
from tests.wide_learner_check import loss_tables as _loss_tables, place_ratios_and_value_steps as _place_ratios_and_value_steps

pytestmark = pytest.mark.gpu

_PARAMS = [pytest.param(nets, shared, mb, gather, id=f"{cid}-mb{mb}")
           for cid, nets, shared in wl.CASES for mb, gather in wl.MB_SMALL] + \
          [pytest.param(nets, shared, wl.MB_LARGE[0], wl.MB_LARGE[1], id=f"{cid}-mb{wl.MB_LARGE[0]}")
           for cid, nets, shared in (wl.CASES[0], wl.CASES[-1])]


def _trainer(spec, shared, mb, gather, seed=5, table_rows=3000):
    """Networks of a case on the device, their input tables (values from randn * 2: both ELU branches in every layer), row list."""
    from legged_games_gym_amd.rl.mlp_kernels import WideMlpTrainer
    nets = [wl.make_mlp(i, h, o, n).cuda() for n, (i, h, o) in enumerate(spec)]
    g = torch.Generator(device="cuda").manual_seed(seed)
    R = table_rows if gather else mb
    xs = [torch.randn(R, spec[0][0], device="cuda", generator=g) * 2.0]
    for i, _, _ in spec[1:]:
        xs.append(xs[0] if shared else torch.randn(R, i, device="cuda", generator=g) * 2.0)
    rows = torch.randperm(R, device="cuda", generator=g)[:mb] if gather else None
    tr = WideMlpTrainer(nets, xs, mb)
    assert tr.supported and not tr.has_fused_minibatch
    return tr, nets, xs, rows, g


def _nan_grads(nets):
    for net in nets:
        for p in net.parameters():
            p.grad = torch.full_like(p, float("nan"))            # the kernels overwrite every element


@pytest.mark.parametrize("precision", [1, 0])
@pytest.mark.parametrize("spec,shared,mb,gather", _PARAMS)
def test_wide_kernels_match_float64_autograd_on_the_generic_path(spec, shared, mb, gather, precision):
    """lg_mlp_wide_forward / lg_mlp_wide_backward against float64 autograd on deep copies of the same modules, for every row of
    wide_learner_check.CASES at both lg_mlp_wide_set_precision settings.  Tolerances: the ones stated per precision for the 235 / 169
    networks (outputs 2e-5 | 1e-4 absolute, gradients 1e-4 | 3e-4 of each tensor's max + 1e-10).  The [observed] line also carries
    the error of torch's own float32 forward / autograd on the same modules, for scale."""
    from legged_games_gym_amd import capi
    lib = capi.load_library()
    if precision == 1:                                             # k_gemm_wide_bf16x3<FWD> must be what runs: the chain kernel cannot be reached
        assert wl.takes_generic_forward(spec)
        assert any((i + 15) // 16 not in (11, 15) or tuple(h) != wl.GAME_HIDDEN or o > 16 for i, h, o in spec) or len({(i + 15) // 16 for i, _, _ in spec}) > 1
    old = lib.lg_mlp_wide_set_precision(precision)
    try:
        tr, nets, xs, rows, g = _trainer(spec, shared, mb, gather)
        refs = [wl.float64_copy(n) for n in nets]
        xb = [(x[rows] if gather else x[:mb]) for x in xs]
        for n, (r, x) in enumerate(zip(refs, xb)):
            wl.assert_both_elu_branches(r, x.double(), f"net {n}")
        want_out = [r(x.double()) for r, x in zip(refs, xb)]
        f32_out = [n(x) for n, x in zip(nets, xb)]
        d_out = [torch.randn(mb, o, device="cuda", generator=g) / mb for _, _, o in spec]
        torch.autograd.backward(want_out, [d.double() for d in d_out])
        torch.autograd.backward(f32_out, d_out)
        want = [p.grad.clone() for r in refs for p in r.parameters()]
        f32_grads = [p.grad.clone() for n in nets for p in n.parameters()]
        f32_err = (wl.max_error(f32_out, want_out, False), wl.max_error(f32_grads, want, True))

        _nan_grads(nets)
        tr.refresh()
        for o in tr.outputs:
            o.fill_(float("nan"))
        outs = tr.forward(rows)
        for buf, d in zip(tr.grad_outputs, d_out):
            buf.copy_(d)
        tr.backward(rows)
        got = [p.grad for n in nets for p in n.parameters()]
        labels = wl.param_labels(nets)
        print(f"[observed] wide {[(i, *h, o) for i, h, o in spec]} mb {mb} precision {precision}: "
              f"outputs {wl.max_error(outs, want_out, False):.3g} (torch f32 {f32_err[0]:.3g}), "
              f"gradients {wl.max_error(got, want, True):.3g} of max (torch f32 {f32_err[1]:.3g})")
        wl.compare_all([f"net{n}.output" for n in range(len(nets))], outs, [w.detach() for w in want_out], abs_tol=wl.OUT_TOL[precision])
        wl.compare_all(labels, got, want, rel=wl.GRAD_TOL[precision], abs_tol=wl.GRAD_ABS)
        first = [h.clone() for h in got] + [o.clone() for o in outs]          # fixed reduction order: bit-reproducible
        tr.forward(rows); tr.backward(rows)
        assert all(torch.equal(a, b) for a, b in zip(first, got + list(outs)))
    finally:
        lib.lg_mlp_wide_set_precision(old)


def _lg_ppo_loss(lib, mu, std, val, ix, t, clip, vc, ec, clipped, d_mu, d_val):
    A, mb = mu.shape[1], mu.shape[0]
    d_std, stats = torch.full((A,), float("nan"), device="cuda"), torch.full((4,), float("nan"), device="cuda")
    p = lambda x: x.data_ptr()
    rc = lib.lg_ppo_loss(p(mu), p(std), p(val), p(ix), p(t["actions"]), p(t["old_lp"]), p(t["old_mu"]), p(t["old_sigma"]), p(t["adv"]), p(t["old_val"]),
                         p(t["ret"]), clip, vc, ec, clipped, p(d_mu), p(d_std), p(d_val), p(stats), mb, A, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.lg_last_error()
    return d_std, stats


@pytest.mark.parametrize("clipped", [1, 0])
@pytest.mark.parametrize("A", [1, 2, 4, 6, 16])
def test_ppo_loss_kernel_matches_float64_at_the_games_action_counts(A, clipped):
    """lg_ppo_loss (k_ppo_loss) against the reference's loss expression evaluated in float64 on .double() copies of the same inputs:
    action counts of the game tasks (idle lanes of the 16-lane row group for A < 16, none for 16), old_sigma different per action and
    different from the current std, mb = 64 * 3 + 5 (a partial last workgroup and a partial last 16-row pass).  Tolerances of
    test_fused_ppo_loss_matches_autograd: stats 2e-5 * max(1, |ref|); gradients 1e-4 of the tensor's max + 1e-6 (d_value: 1e-7)."""
    from legged_games_gym_amd import capi
    lib = capi.load_library()
    R, mb, clip, vc, ec = 400, 64 * 3 + 5, 0.2, 1.0, 0.01
    g = torch.Generator(device="cuda").manual_seed(100 * A + clipped)
    t = _loss_tables(A, R, g)
    ix = torch.randperm(R, device="cuda", generator=g)[:mb]
    mu = t["old_mu"][ix] + 0.3 * torch.randn(mb, A, device="cuda", generator=g)
    std = 0.5 + 1.0 * torch.rand(A, device="cuda", generator=g)
    assert float((std - t["old_sigma"][0]).abs().min()) > 1e-3
    val = torch.randn(mb, 1, device="cuda", generator=g) * 0.3
    _place_ratios_and_value_steps(t, ix, mu, std, val, g, clip)

    def reference(dtype):
        c = lambda x: x.to(dtype)
        leaves = [c(mu).requires_grad_(), c(std).requires_grad_(), c(val).requires_grad_()]
        s, v, kl, ent, ratio, dv = wl.ppo_loss(*leaves, *(c(t[k][ix]) for k in ("actions", "old_lp", "old_mu", "old_sigma", "adv", "old_val", "ret")), clip, clipped)
        (s + vc * v - ec * ent).backward()
        return torch.stack((s, v, kl, ent)).detach(), [l.grad for l in leaves], ratio, dv
    ref, (g_mu, g_std, g_val), ratio, dv = reference(torch.float64)
    wl.assert_loss_inputs_not_degenerate(ratio, dv, clip)
    f32_stats, f32_grads, _, _ = reference(torch.float32)

    d_mu, d_val = torch.full((mb, A), float("nan"), device="cuda"), torch.full((mb, 1), float("nan"), device="cuda")
    d_std, stats = _lg_ppo_loss(lib, mu, std, val, ix, t, clip, vc, ec, clipped, d_mu, d_val)
    print(f"[observed] ppo_loss A {A} clipped {clipped}: stats {wl.max_error([stats], [ref], False):.3g} (torch f32 {wl.max_error([f32_stats], [ref], False):.3g}), "
          f"d_mu {wl.max_error([d_mu], [g_mu], True):.3g}, d_value {wl.max_error([d_val], [g_val], True):.3g}, d_std {wl.max_error([d_std], [g_std], True):.3g} of max "
          f"(torch f32 {wl.max_error(f32_grads, [g_mu, g_std, g_val], True):.3g})")
    wl.compare("stats", stats, ref, abs_tol=2e-5 * max(1.0, float(ref.abs().max())))
    wl.compare("d_mu", d_mu, g_mu, rel=1e-4, abs_tol=1e-6)
    wl.compare("d_value", d_val, g_val, rel=1e-4, abs_tol=1e-7)
    wl.compare("d_std", d_std, g_std, rel=1e-4, abs_tol=1e-6)


@pytest.mark.parametrize("precision", [1, 0])
def test_composed_minibatch_step_matches_float64_autograd_at_the_game_shape(precision):
    """forward -> lg_ppo_loss -> backward of one WideMlpTrainer (actor 19 -> 6, critic 19 -> 1, one observation table, 516 gathered rows)
    against float64 autograd of the WHOLE loss, observations to parameters: every parameter gradient and d loss / d std, with the
    gradient tolerances of the per-layer test (1e-4 | 3e-4 of each tensor's max + 1e-10)."""
    from legged_games_gym_amd import capi
    lib = capi.load_library()
    spec, mb, clip, vc, ec, A = wl.CASES[0][1], 516, 0.2, 1.0, 0.01, 6
    old = lib.lg_mlp_wide_set_precision(precision)
    try:
        tr, nets, xs, ix, g = _trainer(spec, True, mb, True)
        R = xs[0].shape[0]
        std = 0.5 + 1.0 * torch.rand(A, device="cuda", generator=g)
        t = _loss_tables(A, R, g)
        a64, c64 = (wl.float64_copy(n) for n in nets)
        std64 = std.double().requires_grad_()
        xb = xs[0][ix].double()
        mu64, val64 = a64(xb), c64(xb)
        _place_ratios_and_value_steps(t, ix, mu64.detach(), std, val64.detach(), g, clip)
        s, v, kl, ent, ratio, dv = wl.ppo_loss(mu64, std64, val64, *(t[k][ix].double() for k in ("actions", "old_lp", "old_mu", "old_sigma", "adv", "old_val", "ret")), clip, 1)
        wl.assert_loss_inputs_not_degenerate(ratio, dv, clip, margin=1e-2)       # the networks' own error moves the ratio: a wider margin
        (s + vc * v - ec * ent).backward()
        want = [p.grad for r in (a64, c64) for p in r.parameters()]

        _nan_grads(nets)
        tr.refresh()
        mu, val = tr.forward(ix)
        d_std, stats = _lg_ppo_loss(lib, mu, std, val, ix, t, clip, vc, ec, 1, tr.grad_outputs[0], tr.grad_outputs[1])
        tr.backward(ix)
        got = [p.grad for n in nets for p in n.parameters()]
        print(f"[observed] composed step 19-512-256-128-6|1 mb {mb} precision {precision}: gradients {wl.max_error(got, want, True):.3g}, "
              f"d_std {wl.max_error([d_std], [std64.grad], True):.3g} of max, stats {wl.max_error([stats], [torch.stack((s, v, kl, ent))], False):.3g}")
        wl.compare_all(wl.param_labels(nets), got, want, rel=wl.GRAD_TOL[precision], abs_tol=wl.GRAD_ABS)
        wl.compare("d_std", d_std, std64.grad, rel=wl.GRAD_TOL[precision], abs_tol=wl.GRAD_ABS)
    finally:
        lib.lg_mlp_wide_set_precision(old)


def test_after_optimizer_load_drops_the_data_parallel_graphs(monkeypatch):
    """A checkpoint load replaces Adam's state tensors: the captured data-parallel "pre" / "post" graphs (which hold the old
    addresses) and their key must go, like the single-process update graph, its ``whole`` flag and the MlpTrainer's descriptors --
    EVERYTHING captured, through the one invalidation point, from each of the four places that call it."""
    from legged_games_gym_amd.rl import ActorCritic, PPO, ppo
    torch.manual_seed(0)
    ac = ActorCritic(19, 19, 6, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128])
    alg = PPO(ac, schedule="adaptive", desired_kl=0.01, learning_rate=1e-3, device="cuda:0")
    alg.init_storage(16, 4, [19], [None], [6])
    sentinel = (["pre"], "post")

    def seed():
        alg._graph, alg._graph_whole, alg._dp_graphs, alg._dp_key, alg._mlp, alg._updates_done = object(), True, sentinel, ("key",), object(), 3

    def dropped(updates_done):
        return (alg._graph is None and alg._graph_whole is False and alg._dp_graphs is None and alg._dp_key is None and alg._mlp is None
                and alg._updates_done == updates_done)
    seed()
    alg._drop_captured(warm_up_again=False)
    assert dropped(3)
    seed()                                                                  # 1. the checkpoint load: the warm-up starts again
    alg.optimizer.load_state_dict(alg.optimizer.state_dict())
    alg.after_optimizer_load()
    assert dropped(0)
    assert alg.optimizer.param_groups[0]["lr"] is alg._lr
    seed()                                                                  # 2. a rebuild of the flat gradient buffer
    flat = alg._flat_grad_views()
    assert dropped(3)
    # steady state: the buffer is kept, and so is what was captured over it; its address and Adam's state addresses are part of the key
    seed()
    assert alg._flat_grad_views() is flat and alg._dp_graphs is sentinel and alg._graph is not None and alg._dp_key == ("key",)
    assert alg._dp_state_key()[-1] == flat.data_ptr() and alg._capture_key(64)[4:] == alg._dp_state_key()
    alg._begin_update(None)                                                 # 3. the key check of an update, one process: warm up again
    assert alg._graph is None and alg._graph_whole is False and alg._dp_graphs is None and alg._mlp is None and alg._updates_done == 0
    assert alg._dp_key == alg._capture_key(64)
    seed()                                                                  # 4. ... and of a data-parallel update: captured again at once
    monkeypatch.setattr(ppo, "_world", lambda: 2)
    alg._begin_update(None)
    assert alg._graph is None and alg._graph_whole is False and alg._dp_graphs is None and alg._mlp is None and alg._updates_done == 3
    # nothing captured: a key that moves (Adam's state appears during the first update) restarts nothing
    alg._dp_key, alg._updates_done = ("key",), 1
    alg._begin_update(None)
    assert alg._updates_done == 1 and alg._dp_key == alg._capture_key(64)


def _dp_resume_worker(rank, world, port, out):
    """One data-parallel rank: learn, save, load, learn -- with the two-graph update and, from the same start, with eager launches."""
    import torch.distributed as dist
    from legged_games_gym_amd import capi
    from legged_games_gym_amd.rl import ActorCritic, PPO
    from tests.test_gpu_rl import _storage
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    capi.load_library().lg_mlp_wide_set_precision(0)
    obs, A, T, N = 19, 6, 8, 128
    result = {}
    for graphs in ("1", "0"):
        os.environ["LG_DP_GRAPHS"] = graphs
        torch.manual_seed(0)
        ac = ActorCritic(obs, obs, A, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[512, 256, 128])
        alg = PPO(ac, num_learning_epochs=1, num_mini_batches=2, schedule="adaptive", desired_kl=0.01, learning_rate=1e-3, entropy_coef=0.01, device="cuda:0")
        alg.init_storage(N, T, [obs], [None], [A])
        launches = []

        def learn(first):
            for it in range(first, first + 3):               # eager, capture + replay, replay
                _storage(T=T, N=N, seed=100 * it + rank, st=alg.storage, obs=obs, act=A)
                alg.storage.compute_returns(torch.zeros(N, 1, device="cuda"), 0.99, 0.95)
                alg.update(perm=torch.randperm(T * N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(it)))
                launches.append(alg.dp_launches)
        learn(0)
        path = f"{out}/ckpt_{graphs}_r{rank}.pt"
        torch.save({"model": alg.actor_critic.state_dict(), "optimizer": alg.optimizer.state_dict()}, path)
        d = torch.load(path, map_location="cuda:0", weights_only=True)
        alg.actor_critic.load_state_dict(d["model"])
        alg.optimizer.load_state_dict(d["optimizer"])
        alg.after_optimizer_load()
        learn(3)
        steps = sorted({float(s["step"]) for s in alg.optimizer.state.values()})
        result[graphs] = {"params": [p.detach().cpu().clone() for p in alg.actor_critic.parameters()], "lr": alg.learning_rate, "launches": launches,
                          "steps": steps, "graph_error": getattr(alg, "_dp_graph_error", None), "wide": alg._mlp is not None and not alg._mlp.has_fused_minibatch}
    torch.save(result, f"{out}/r{rank}.pt")
    dist.destroy_process_group()


def test_data_parallel_update_after_a_checkpoint_load_equals_the_eager_one(tmp_path):
    """Two gloo ranks on the one GPU, game-shaped networks (wide kernels): three updates, save, load, three updates.  The run whose
    updates replay the captured "pre" / "post" graphs must end where the run with eager launches (LG_DP_GRAPHS=0) ends -- after the load
    the graphs are captured again over the new Adam state -- by the criterion of test_data_parallel_kernel_update_two_ranks_one_gpu."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_dp_resume_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f"r{k}.pt", weights_only=True) for k in (0, 1))
    replayed = {"graph_replays": 4, "collectives": 2, "kernel_launches_from_host": 0}
    assert r0["1"]["graph_error"] is None and r0["1"]["wide"] and r0["0"]["wide"]
    assert r0["1"]["launches"] == [None, replayed, replayed] * 2, r0["1"]["launches"]      # eager again after the load, then re-captured
    assert r0["0"]["launches"] == [None] * 6
    assert r0["1"]["steps"] == r0["0"]["steps"] == [12.0]                                  # the LOADED Adam state is the one that moved on
    for a, b in zip(r0["1"]["params"], r1["1"]["params"]):
        assert torch.equal(a, b)                                                           # replicas stay bit-identical
    for got, want in zip(r0["1"]["params"], r0["0"]["params"]):
        d = (want - got).abs()
        assert float((d > 2e-6 + 2e-4 * got.abs()).float().mean()) < 1e-3 and float(d.max()) <= 2.1e-3, (float(d.max()), float((d > 2e-6).float().mean()))
    assert abs(r0["1"]["lr"] - r0["0"]["lr"]) < 1e-9
