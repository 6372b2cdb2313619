"""The structure ``rl/ppo.py`` promises: every attribute of ``PPO`` and ``RolloutStorage`` is declared by its constructor (an update adds
none, on any path), the loss / KL bodies every path shares are the expressions they replaced bit for bit, and a re-allocated storage
is picked up by the captured update."""
import copy

import pytest
import torch

from legged_games_gym_amd.rl import PPO, ActorCritic
from legged_games_gym_amd.rl.ppo import gaussian_kl


def _attribute_sets(alg):
    return sorted(vars(alg)), sorted(vars(alg.storage))


@pytest.mark.parametrize("recurrent", [False, True])
def test_an_update_adds_no_attribute_cpu(recurrent):
    from tests.test_recurrent_policy import StubEnv, _collect, _policy, _scripted
    N, T, I, A = 6, 8, 10, 3
    torch.manual_seed(0)
    ac = _policy(I=I, Ic=I, A=A) if recurrent else ActorCritic(I, I, A, actor_hidden_dims=[16], critic_hidden_dims=[16])
    alg = PPO(ac, num_learning_epochs=2, num_mini_batches=2, schedule="adaptive", desired_kl=0.01, device="cpu")
    alg.init_storage(N, T, [I], [None], [A])
    declared = _attribute_sets(alg)
    last = _collect(alg, StubEnv(N, I, A, _scripted(N, T)), T)
    with torch.inference_mode():
        alg.compute_returns(last)
    alg.update()
    assert _attribute_sets(alg) == declared


def _parent_loss(lp, old_lp, adv, val, tval, ret, ent, clip, vc, ec, clipped, squeeze):
    """The expression ``_mb_step`` (``torch.squeeze``) and the eager loop of ``update`` (``.squeeze(-1)``) each spelled out before."""
    ratio = torch.exp(lp - squeeze(old_lp))
    a = squeeze(adv)
    surrogate = torch.max(-a * ratio, -a * torch.clamp(ratio, 1.0 - clip, 1.0 + clip)).mean()
    if clipped:
        vclip = tval + (val - tval).clamp(-clip, clip)
        vloss = torch.max((val - ret).pow(2), (vclip - ret).pow(2)).mean()
    else:
        vloss = (ret - val).pow(2).mean()
    return surrogate + vc * vloss - ec * ent.mean(), surrogate, vloss


@pytest.mark.parametrize("clipped", [True, False])
@pytest.mark.parametrize("A", [1, 12])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_shared_loss_and_kl_are_the_parent_expressions_bit_for_bit(dtype, A, clipped):
    g = torch.Generator().manual_seed(A)
    mb, clip, vc, ec = 37, 0.2, 0.7, 0.01
    r = lambda *s: torch.randn(*s, generator=g, dtype=dtype)
    mu, old_mu = r(mb, A), r(mb, A)
    sig, old_sig = 0.5 + torch.rand(mb, A, generator=g, dtype=dtype), 0.5 + torch.rand(mb, A, generator=g, dtype=dtype)
    lp, old_lp, adv = r(mb), r(mb, 1) * 0.3, r(mb, 1)        # ratios on both sides of the clip edges
    lp = lp * 0.3
    val, tval, ret, ent = r(mb, 1), r(mb, 1) + 0.1, r(mb, 1), r(mb)
    alg = PPO(ActorCritic(4, 4, A, actor_hidden_dims=[8], critic_hidden_dims=[8]), clip_param=clip, value_loss_coef=vc, entropy_coef=ec,
              use_clipped_value_loss=clipped, device="cpu")
    for squeeze in (torch.squeeze, lambda t: t.squeeze(-1)):
        want = _parent_loss(lp, old_lp, adv, val, tval, ret, ent, clip, vc, ec, clipped, squeeze)
        got = alg._loss(lp, squeeze(old_lp), squeeze(adv), val, tval, ret, ent)
        assert all(torch.equal(w, h) for w, h in zip(want, got))
    ratio = torch.exp(lp - old_lp.squeeze(-1))
    assert bool((ratio < 1 - clip).any()) and bool((ratio > 1 + clip).any()) and bool(((val - tval).abs() > clip).any())
    want = torch.sum(torch.log(sig / old_sig + 1.0e-5) + (old_sig.square() + (old_mu - mu).square()) / (2.0 * sig.square()) - 0.5, dim=-1)
    assert torch.equal(gaussian_kl(mu, sig, old_mu, old_sig), want)


# ---------------------------------------------------------------------------------------------------------------- on the GPU
OBS, ACT, T, N = 48, 12, 8, 64                # 2 epochs x 4 mini-batches of 128 rows: one full 16-row tile group and the persistent loop's idle waves


def _gpu_alg(graphed=True, ac=None):
    torch.manual_seed(0)
    ac = ac if ac is not None else ActorCritic(OBS, OBS, ACT, actor_hidden_dims=[128, 64, 32], critic_hidden_dims=[128, 64, 32], activation="elu")
    alg = PPO(ac, num_learning_epochs=2, num_mini_batches=4, learning_rate=1e-3, schedule="adaptive", desired_kl=0.01, entropy_coef=0.01,
              device="cuda", graphed_update=graphed)
    alg.init_storage(N, T, [OBS], [None], [ACT])
    return alg


def _gpu_update(alg, it, rank=0):
    from tests.test_gpu_rl import _storage
    st = alg.storage
    n = st.num_envs
    _storage(T=T, N=n, seed=100 * it + rank, st=st)
    st.compute_returns(torch.zeros(n, 1, device="cuda"), 0.99, 0.95)
    return alg.update(torch.randperm(T * n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(it)))


@pytest.mark.gpu
@pytest.mark.parametrize("mlp_kernels", ["1", "0"])
def test_an_update_adds_no_attribute_gpu(monkeypatch, mlp_kernels):
    """Eager warm-up, capture and replay, with the learner kernels (whole-update graph) and on the torch MLP path (one-step graph)."""
    monkeypatch.setenv("LG_PPO_MLP_KERNELS", mlp_kernels)
    alg = _gpu_alg()
    declared = _attribute_sets(alg)
    for it in range(3):
        _gpu_update(alg, it)
        assert _attribute_sets(alg) == declared
    assert alg._graph is not None and alg._graph_whole == (mlp_kernels == "1") and (alg._mlp is not None) == (mlp_kernels == "1")


def _two_rank_worker(rank, world, port, out):
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    alg = _gpu_alg()
    declared = _attribute_sets(alg)
    after = []
    for it in range(3):
        _gpu_update(alg, it, rank)
        after.append(_attribute_sets(alg))
    torch.save({"declared": declared, "after": after, "launches": alg.dp_launches, "graph_error": alg._dp_graph_error,
                "flat": alg._gflat is not None}, f"{out}/r{rank}.pt")
    dist.destroy_process_group()


@pytest.mark.gpu
def test_an_update_adds_no_attribute_two_ranks(tmp_path):
    """Two gloo ranks on the one GPU: eager, capture of the "pre" / "post" graphs, replay."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_two_rank_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    for k in (0, 1):
        r = torch.load(tmp_path / f"r{k}.pt", weights_only=True)
        assert r["graph_error"] is None and r["flat"] and r["launches"] == {"graph_replays": 16, "collectives": 8, "kernel_launches_from_host": 0}
        assert all(a == r["declared"] for a in r["after"])


def _two_rank_resize_worker(rank, world, port, out):
    """Three updates, ``init_storage`` with 96 envs, two more -- with the "pre" / "post" graphs and, from the same start, with eager launches."""
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    result = {}
    for graphs in ("1", "0"):
        os.environ["LG_DP_GRAPHS"] = graphs                  # read by the constructor
        alg = _gpu_alg()
        launches, std_in_flat = [], []
        for it in range(5):
            if it == 3:
                alg.init_storage(96, T, [OBS], [None], [ACT])
            _gpu_update(alg, it, rank)
            launches.append(alg.dp_launches)
            slot = alg._gflat[alg._goffs[[n for n, _ in alg.actor_critic.named_parameters()].index("std")]].data_ptr()
            std_in_flat.append(alg._d_std.data_ptr() == slot and alg.actor_critic.std.grad.data_ptr() == slot)
        result[graphs] = {"params": [p.detach().cpu().clone() for p in alg.actor_critic.parameters()], "lr": alg.learning_rate,
                          "launches": launches, "std_in_flat": std_in_flat, "graph_error": alg._dp_graph_error}
    torch.save(result, f"{out}/r{rank}.pt")
    dist.destroy_process_group()


@pytest.mark.gpu
def test_a_reallocated_storage_on_two_ranks_keeps_the_std_gradient_in_the_flat_buffer(tmp_path):
    """The storage changes size under the data-parallel kernel update: the per-update buffers are allocated again, but d loss / d std must
    stay the std slot of the flat buffer the all-reduce sums -- a rank-local ``_d_std`` would leave ``std`` with an unreduced gradient and
    the replicas (whose shards differ) would part.  The graphs are captured again in the update that meets the new storage, and the run ends
    where the run with eager launches ends, by the criterion of ``test_data_parallel_update_after_a_checkpoint_load_equals_the_eager_one``."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_two_rank_resize_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f"r{k}.pt", weights_only=True) for k in (0, 1))
    replayed = {"graph_replays": 16, "collectives": 8, "kernel_launches_from_host": 0}
    assert r0["1"]["graph_error"] is None and r0["1"]["launches"] == [None] + [replayed] * 4, (r0["1"]["graph_error"], r0["1"]["launches"])
    assert r0["0"]["launches"] == [None] * 5
    for graphs in ("1", "0"):
        assert all(r0[graphs]["std_in_flat"]) and all(r1[graphs]["std_in_flat"])
        for a, b in zip(r0[graphs]["params"], r1[graphs]["params"]):
            assert torch.equal(a, b)                                                       # replicas stay bit-identical
    for got, want in zip(r0["1"]["params"], r0["0"]["params"]):
        d = (want - got).abs()
        assert float((d > 2e-6 + 2e-4 * got.abs()).float().mean()) < 1e-3 and float(d.max()) <= 2.1e-3, (float(d.max()), float((d > 2e-6).float().mean()))
    assert abs(r0["1"]["lr"] - r0["0"]["lr"]) < 1e-9


@pytest.mark.gpu
def test_a_reallocated_storage_is_captured_again():
    """Three graphed updates, ``init_storage`` with 96 envs (mini-batches of 192 rows at new addresses), two more: the graph over the old
    storage goes, an eager warm-up and a new capture follow, and the five updates end where five eager ones end -- by the tolerances of
    ``test_graph_captured_update_equals_the_eager_update``."""
    torch.manual_seed(0)
    ac0 = ActorCritic(OBS, OBS, ACT, actor_hidden_dims=[128, 64, 32], critic_hidden_dims=[128, 64, 32], activation="elu").cuda()
    out = []
    for graphed in (False, True):
        alg = _gpu_alg(graphed, copy.deepcopy(ac0))
        losses = []
        for it in range(5):
            if it == 3:
                old = alg._graph
                alg.init_storage(96, T, [OBS], [None], [ACT])
            losses.append(_gpu_update(alg, it))
            if graphed:
                assert (alg._graph is None) == (it in (0, 3)) and (it != 4 or (alg._graph is not old and alg._graph_whole))
        out.append((losses, [p.detach().clone() for p in alg.actor_critic.parameters()], alg.learning_rate))
    (l_e, p_e, lr_e), (l_g, p_g, lr_g) = out
    assert abs(lr_e - lr_g) < 1e-9 * max(1.0, lr_e) + 1e-12 or abs(lr_e - lr_g) / lr_e < 1e-5
    for (ve, se), (vg, sg) in zip(l_e, l_g):
        assert abs(ve - vg) < 2e-5 and abs(se - sg) < 2e-5
    for a, b in zip(p_e, p_g):
        assert float((a - b).abs().max()) < 1e-4
