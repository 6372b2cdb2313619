"""Shared pieces of tests/test_gpu_wide_learner.py (GPU) and tests/test_wide_learner_check.py (CPU): the got-vs-want comparison the
wide learner tests assert with, the networks and cases they run, and a float64-capable restatement of the PPO loss expression.
Nothing here touches the device library, so the comparison itself is tested without a GPU."""
import copy

import torch
import torch.nn as nn

# tolerances the project states per lg_mlp_wide_set_precision setting (tests/test_gpu_rl.py::_wide_mlp_check):
# outputs absolute; gradients relative to each tensor's largest magnitude, plus 1e-10
OUT_TOL = {0: 2e-5, 1: 1e-4}
GRAD_TOL = {0: 1e-4, 1: 3e-4}
GRAD_ABS = 1e-10

GAME_HIDDEN = (512, 256, 128)
# (id, [(inputs, hidden widths, outputs) per net], both nets read one input tensor) -- from the registered game shapes to the exotic ones
CASES = [
    ("game_19_6_1", [(19, GAME_HIDDEN, 6), (19, GAME_HIDDEN, 1)], True),           # high_level_game: K = 19 padded to 20, narrow output N = 6
    ("dec_prey_16_4_1", [(16, GAME_HIDDEN, 4), (16, GAME_HIDDEN, 1)], True),       # layer 0 an exact multiple of 4: bias column 16 on a quad boundary
    ("dec_pred_3_2_1", [(3, GAME_HIDDEN, 2), (3, GAME_HIDDEN, 1)], True),          # K smaller than one quad: k0p = 4, ldc = 4
    ("sep_19_6_and_16_1", [(19, GAME_HIDDEN, 6), (16, GAME_HIDDEN, 1)], False),    # critic with its own input tensor: per-net k0p / workspace slices
    ("rough_sep_235_12_and_169_1", [(235, GAME_HIDDEN, 12), (169, GAME_HIDDEN, 1)], False),  # chain refused (k-steps 15 vs 11): the FWD GEMMs at the rough widths
    ("single_19_16", [(19, GAME_HIDDEN, 16)], False),                              # k_wide_out_bwd at N = LG_OUT_MAXN, one net: n_nets = 1 reduce jobs
    ("single_19_17", [(19, GAME_HIDDEN, 17)], False),                              # first shape past it: generic dW / dX on the output layer
    ("ragged_45_132_50_30_7", [(45, (132, 50, 30), 7)], False),                    # no width a multiple of 128 / 32; C strides 50 / 30: scalar-store epilogue
]
# (mini-batch rows, gathered through a row list): chosen for the kernels' branches
MB_SMALL = [(37, False), (516, True)]      # less than one tile, mb % 4 != 0 | mb % 4 == 0 (the `fast` loops), four row tiles + a 4-row tail
MB_LARGE = (2049, True)                    # out_chunks = 256 with empty trailing chunks; a last dW split of one row


def make_mlp(num_in, hidden, num_out, seed):
    """Linear-ELU-Linear-ELU-Linear-ELU-Linear, torch's default initialisation from ``seed`` (CPU; the caller moves it)."""
    torch.manual_seed(seed)
    dims = [num_in] + list(hidden)
    mods = []
    for a, b in zip(dims[:-1], dims[1:]):
        mods += [nn.Linear(a, b), nn.ELU()]
    return nn.Sequential(*mods, nn.Linear(dims[-1], num_out))


def takes_generic_forward(nets):
    """The host rule of lg_mlp_wide_forward at precision 1, restated: the chain kernel needs 512-256-128 hidden widths, <= 16 outputs,
    ceil(inputs / 16) in {11, 15} for every net AND the same number of layer-0 k-steps in both; anything else runs the per-layer GEMMs."""
    steps = [(i + 15) // 16 for i, _, _ in nets]
    chain = all(tuple(h) == GAME_HIDDEN and o <= 16 and s in (11, 15) for (_, h, o), s in zip(nets, steps)) and len(set(steps)) == 1
    return not chain


def compare(label, got, want, rel=0.0, abs_tol=0.0):
    """THE check of the wide learner tests: every element of ``got`` finite and max |got - want| < rel * max |want| + abs_tol, in float64.
    Returns the error as a fraction of the bound's scale (max |want| when rel > 0, else absolute)."""
    assert got.shape == want.shape, f"{label}: shape {tuple(got.shape)} against {tuple(want.shape)}"
    g, w = got.detach().double().cpu(), want.detach().double().cpu()
    assert bool(torch.isfinite(g).all()), f"{label}: {int((~torch.isfinite(g)).sum())} non-finite elements (not overwritten?)"
    err, scale = float((g - w).abs().max()), float(w.abs().max())
    bound = rel * scale + abs_tol
    assert err < bound, f"{label}: max error {err:.3e} >= {bound:.3e} (rel {rel:g} of max {scale:.3e} + {abs_tol:g})"
    return err / scale if rel > 0.0 and scale > 0.0 else err


def compare_all(labels, got, want, rel=0.0, abs_tol=0.0):
    """``compare`` over lists of tensors; the largest figure."""
    assert len(got) == len(want) == len(labels)
    return max(compare(l, g, w, rel, abs_tol) for l, g, w in zip(labels, got, want))


def max_error(got, want, relative):
    """Largest error of a list of tensors against the float64 ones, no assertion (the float32-torch figures printed beside the kernel's)."""
    out = 0.0
    for g, w in zip(got, want):
        e = float((g.detach().double() - w.detach().double()).abs().max())
        out = max(out, e / (float(w.abs().max()) + 1e-300) if relative else e)
    return out


def param_labels(nets):
    return [f"net{n}.{name}.grad" for n, net in enumerate(nets) for name, _ in net.named_parameters()]


def float64_copy(net):
    return copy.deepcopy(net).double()


def assert_both_elu_branches(net64, x64, label, share=0.10):
    """On the float64 reference: every hidden layer has at least ``share`` of its activations on each side of 0."""
    h = x64
    with torch.no_grad():
        for m in net64:
            h = m(h)
            if isinstance(m, nn.ELU):
                pos = float((h > 0).double().mean())
                assert share <= pos <= 1.0 - share, f"{label}: a hidden layer has {pos:.3f} of its activations above 0"


def ppo_loss(mu, std, val, act, old_lp, old_mu, old_sigma, adv, old_val, ret, clip, clipped_value):
    """The reference's PPO loss terms (rsl_rl PPO.update, as in test_fused_ppo_loss_matches_autograd) in the dtype of the inputs.
    Returns surrogate, value loss, KL, entropy and the per-row ratio / value step (for the inputs' non-degeneracy checks)."""
    dist_ = torch.distributions.Normal(mu, mu * 0.0 + std)
    lp = dist_.log_prob(act).sum(-1)
    ratio = torch.exp(lp - old_lp.squeeze(-1))
    a = adv.squeeze(-1)
    surrogate = torch.max(-a * ratio, -a * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
    if clipped_value:
        vclip = old_val + (val - old_val).clamp(-clip, clip)
        vloss = torch.max((val - ret).pow(2), (vclip - ret).pow(2)).mean()
    else:
        vloss = (ret - val).pow(2).mean()
    ent = dist_.entropy().sum(-1).mean()
    kl = torch.sum(torch.log(std / old_sigma + 1e-5) + (old_sigma.square() + (old_mu - mu).square()) / (2.0 * std.square()) - 0.5, dim=-1).mean()
    return surrogate, vloss, kl, ent, ratio.detach(), (val - old_val).detach().squeeze(-1)


def assert_loss_inputs_not_degenerate(ratio, dv, clip, share=0.20, margin=1e-3):
    """On the reference alone: at least ``share`` of the rows inside and outside the ratio clip range and on each side of the value
    clip, and no row within ``margin`` of an edge (there a rounding error of the kernel would legitimately pick the other branch)."""
    inside = ((ratio >= 1 - clip) & (ratio <= 1 + clip)).double().mean()
    assert share <= float(inside) <= 1 - share, f"{float(inside):.3f} of the rows have the ratio inside the clip range"
    v_in = (dv.abs() <= clip).double().mean()
    assert share <= float(v_in) <= 1 - share, f"{float(v_in):.3f} of the rows have the value step inside the clip range"
    edge = torch.minimum((ratio - (1 - clip)).abs(), (ratio - (1 + clip)).abs()).min()
    assert float(edge) > margin and float((dv.abs() - clip).abs().min()) > margin, "a row sits on a clip edge"


def spread(gen, n, lo, edges, hi, gap, device, dtype=torch.float64):
    """n values uniform on [lo, hi]; a value closer than ``gap`` to one of ``edges`` is moved ``gap`` further away from it."""
    u = lo + (hi - lo) * torch.rand(n, device=device, generator=gen, dtype=dtype)
    for e in edges:
        near = (u - e).abs() < gap
        u = torch.where(near, torch.where(u >= e, e + gap + (u - e), e - gap + (u - e)), u)
    return u


def loss_tables(A, R, g, dev="cuda"):
    """Storage-like tables of R rows (float32, as RolloutStorage holds them): old_sigma varies per action and is the same in every row."""
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    old_sigma = (0.4 + 1.2 * torch.rand(A, device=dev, generator=g)).expand(R, A).contiguous()
    old_mu = r(R, A) * 0.2
    t = dict(old_sigma=old_sigma, old_mu=old_mu, actions=old_mu + old_sigma * r(R, A), adv=r(R, 1), old_val=r(R, 1) * 0.3)
    t["ret"] = t["old_val"] + 0.5 * r(R, 1)
    return t


def place_ratios_and_value_steps(t, ix, mu, std, val, g, clip):
    """old_log_prob / old values of the mini-batch rows, set from the float64 reference's own log-probability and value so that the
    ratio is uniform on [1 - 2 clip, 1 + 2 clip] and the value step on [-2 clip, 2 clip], nothing within 0.02 of a clip edge (a stored
    log-probability under ANOTHER sigma would put every row of a 16-action policy far outside the range)."""
    mb = ix.numel()
    dist_ = torch.distributions.Normal(mu.double(), mu.double() * 0.0 + std.double())
    lp = dist_.log_prob(t["actions"][ix].double()).sum(-1)
    u = spread(g, mb, 1 - 2 * clip, (1 - clip, 1 + clip), 1 + 2 * clip, 0.02, mu.device)
    dv = spread(g, mb, -2 * clip, (-clip, clip), 2 * clip, 0.02, mu.device)
    old_lp = torch.zeros(t["adv"].shape[0], 1, device=mu.device)
    old_lp[ix, 0] = (lp - torch.log(u)).float()
    t["old_val"][ix, 0] = (val.double().squeeze(-1) - dv).float()
    t["ret"][ix] = t["old_val"][ix] + 0.5 * torch.randn(mb, 1, device=mu.device, generator=g)
    t["old_lp"] = old_lp
