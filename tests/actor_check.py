"""Shared pieces of tests/test_gpu_actor_edges.py (GPU) and tests/test_actor_check.py (CPU): the host rule of lg_policy_act
(csrc/lg_learner.hip) restated, the case table that takes each of the nine stand-alone actor kernels (csrc/lg_policy.h) to its edges,
the float64 reference, a float64 model of the split-bf16 arithmetic of the wide build, and the bars.  CPU torch only; nothing here touches
the device library, so the table's reach claims and the bars' controls are tested without a GPU.

Edges: the first, a middle and the last observation width of each instantiation's tile range (zero padding inside the last 16-wide
tile, in the kernel and in both pack paths); env counts on every side of a workgroup (16 envs exact, 32 split-bf16: idle lanes re-read env
N - 1) and, for the split-bf16 kernels, 1000 envs = 32 workgroups, one per k-step rotation, the last ragged; action counts that end
inside and on a lane group of four (1, 4, 5, 12, 13, 16)."""
import functools
import types
from collections import namedtuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import wide_learner_check as wl

FLAT_HIDDEN, WIDE_HIDDEN = (128, 64, 32), wl.GAME_HIDDEN
EXACT_TOL = 2e-5                         # TOL of tests/test_gpu_recurrent.py: the exact-f32 MFMA kernels
SPLIT_TOL = wl.OUT_TOL[1]                # 1e-4: the split-bf16 build
ACTIONS = (1, 4, 5, 12, 13, 16)
REGIMES = ("default", "x3", "obs100")    # default nn.Linear weights, obs = randn * 2 | every parameter x 3 | obs = randn * 100 (clip_observations)
ROTATIONS = 32                           # k-steps of layer 1's input in the wide build: r1 = (blk * 5) % 32

# build: "exact" (k_policy_act<tiles, ...>, 16 envs per workgroup) | "wide" (k_policy_act_wide<tiles, 16, 8, 4>, 32 envs per workgroup)
# precision: what lg_mlp_wide_set_precision must hold for lg_policy_act to dispatch this kernel (None: either)
Kernel = namedtuple("Kernel", "name build tiles hidden widths wg_envs precision envs")
Case = namedtuple("Case", "id kernel num_obs num_actions num_envs regime seed")

_EXACT_ENVS, _WIDE_ENVS = (1, 15, 16, 17), (1, 31, 32, 33, 1000)
_RANGES = {3: (33, 47, 48), 15: (225, 235, 240), 11: (161, 169, 176), 2: (17, 19, 32), 1: (1, 3, 16)}
KERNELS = tuple(
    [Kernel("exact3", "exact", 3, FLAT_HIDDEN, _RANGES[3], 16, None, _EXACT_ENVS)]
    + [Kernel(f"exact{t}", "exact", t, WIDE_HIDDEN, _RANGES[t], 16, 0, _EXACT_ENVS) for t in (15, 11, 2, 1)]
    + [Kernel(f"wide{t}", "wide", t, WIDE_HIDDEN, _RANGES[t], 32, 1, _WIDE_ENVS) for t in (15, 11, 2, 1)])

# (index into the kernel's widths, actions, index into its env counts, regime): not the cross product -- every width, action count, env
# count and regime at least once per kernel, 16 actions on a ragged env count with the nearly empty AND the full last tile.  The default
# regime stays off the rows with 17 outputs or fewer: over so few elements a lost cross term is 7 .. 10 split bars, not the > 10 of the
# control in tests/test_actor_check.py; with 64 or more it is 13 or more, whatever the seed
_PATTERN = (
    (0, 1, 3, "x3"),                     # first width of the range, one action, one env past a workgroup
    (1, 4, 2, "default"),                # an exact multiple of everything
    (2, 5, 1, "obs100"),                 # last width, one env short
    (0, 12, 0, "obs100"),                # a single env
    (1, 13, 3, "default"),
    (2, 16, 1, "x3"),                    # full last tile, all four action groups, ragged
    (0, 16, 3, "default"),               # nearly empty last tile, all four action groups, one env in the second workgroup
    (2, 13, 0, "obs100"),
    (0, 5, 2, "x3"),
    (1, 12, 1, "obs100"),
)
_PATTERN_WIDE = ((1, 16, 4, "default"), (2, 1, 4, "x3"))       # 1000 envs: every rotation of the weight stream, the last workgroup ragged


def _cases():
    out = []
    for k in KERNELS:
        for wi, na, ei, regime in _PATTERN + (_PATTERN_WIDE if k.build == "wide" else ()):
            w, n = k.widths[wi], k.envs[ei]
            out.append(Case(f"{k.name}-obs{w}-act{na}-N{n}-{regime}", k, w, na, n, regime, len(out)))
    return tuple(out)


CASES = _cases()
CASE_IDS = tuple(c.id for c in CASES)
# what lg_policy_act must refuse with -4 (hidden widths, observations), and what lg_policy_create must (dims[0..4])
REFUSED_AT_ACT = tuple((WIDE_HIDDEN, o) for o in (33, 160, 177, 224, 241)) + tuple((FLAT_HIDDEN, o) for o in (32, 49))
REFUSED_AT_CREATE = ((257,) + WIDE_HIDDEN + (12,), (48,) + FLAT_HIDDEN + (17,), (48, 128, 24, 32, 12))
# first and last width of every range, per kernel: host pack against device pack at the padded widths
REPACK = tuple((k, w) for k in KERNELS for w in (k.widths[0], k.widths[-1]))


def case(cid):
    return CASES[CASE_IDS.index(cid)]


def kernel_for(hidden, num_obs, precision):
    """lg_policy_act's dispatch restated: the name of the kernel in KERNELS, or None where the call is refused with -4."""
    t0 = (num_obs + 15) // 16
    if tuple(hidden) == WIDE_HIDDEN and t0 in (15, 11, 2, 1):
        return f"{'wide' if precision == 1 else 'exact'}{t0}"
    if tuple(hidden) == FLAT_HIDDEN and t0 == 3:
        return "exact3"
    return None


def workgroups(c):
    return (c.num_envs + c.kernel.wg_envs - 1) // c.kernel.wg_envs


def ragged(c):
    return c.num_envs % c.kernel.wg_envs != 0


def rotations(c):
    """Layer-1 k-step rotations the workgroups of a wide case start their ring at."""
    return {(5 * b) % ROTATIONS for b in range(workgroups(c))}


def tol(kernel):
    return EXACT_TOL if kernel.build == "exact" else SPLIT_TOL


def make_inputs(num_obs, hidden, num_actions, num_envs, regime, seed):
    """(actor, obs, std): Linear / ELU x 3 / Linear in float32 on the CPU, ``obs`` [num_envs, num_obs] float32, a distinct std per action."""
    net = wl.make_mlp(num_obs, hidden, num_actions, seed)
    g = torch.Generator().manual_seed(1000 + seed)
    obs = torch.randn(num_envs, num_obs, generator=g) * (100.0 if regime == "obs100" else 2.0)
    if regime == "x3":
        with torch.no_grad():
            for p in net.parameters():
                p.mul_(3.0)
    assert regime in REGIMES
    return net, obs, torch.linspace(0.3, 1.4, num_actions)


def float64_forward(net, obs, label=None):
    """The float64 copy of ``net`` on ``obs``; with a ``label``, both ELU branches must be live in every hidden layer."""
    net64, x = wl.float64_copy(net), obs.detach().double().cpu()
    if label is not None:
        wl.assert_both_elu_branches(net64, x, label)
    with torch.no_grad():
        return net64(x)


def _split(x32):
    hi = x32.to(torch.bfloat16).float()
    lo = (x32 - hi).to(torch.bfloat16).float()
    return hi.double(), lo.double()


def split_bf16_forward64(net, obs, cross=True):
    """The arithmetic csrc/lg_policy.h documents for the wide build, accumulated in float64: every float32 operand x is hi = bf16(x),
    lo = bf16(x - hi); a product is hi*hi + hi*lo + lo*hi (lo*lo dropped); bias and ELU on the sum; activations rounded to float32
    between layers.  ``cross=False`` keeps hi*hi only: what a kernel that loses its cross terms computes."""
    lin = [m for m in net if isinstance(m, nn.Linear)]
    h = obs.detach().float().cpu()
    with torch.no_grad():
        for i, m in enumerate(lin):
            xh, xl = _split(h)
            wh, wlo = _split(m.weight.detach().float().cpu())
            y = xh @ wh.T
            if cross:
                y = y + xh @ wlo.T + xl @ wh.T
            y = y + m.bias.detach().double().cpu()
            if i + 1 < len(lin):
                h = F.elu(y).float()
    return y


def zeroed_last_column(net, obs):
    """Float64 forward of what a kernel sees that pads one observation column too many."""
    x = obs.clone()
    x[:, -1] = 0.0
    return float64_forward(net, x)


def swapped_action_rows(net, obs):
    """Float64 forward with the last two rows of the output layer exchanged (weights and biases): a lost or misplaced action lane.
    For 5 and 13 actions the pair straddles two lane groups.  None for a single action."""
    out = [m for m in net if isinstance(m, nn.Linear)][-1]
    n = out.out_features
    if n < 2:
        return None
    bad = wl.float64_copy(net)
    last = [m for m in bad if isinstance(m, nn.Linear)][-1]
    with torch.no_grad():
        last.weight[[n - 2, n - 1]] = last.weight[[n - 1, n - 2]]
        last.bias[[n - 2, n - 1]] = last.bias[[n - 1, n - 2]]
        return bad(obs.double())


def max_err(got, want):
    return float((got.detach().double().cpu() - want).abs().max())


@functools.lru_cache(maxsize=None)
def reference(cid):
    """Inputs, float64 means and the controls' errors of a case: computed once, never modified.  ``control`` is the error of the
    arithmetic the kernel is supposed to do, carried out on the CPU: float32 torch for the exact kernels, the split-bf16 model for the
    wide ones."""
    c = case(cid)
    net, obs, std = make_inputs(c.num_obs, c.kernel.hidden, c.num_actions, c.num_envs, c.regime, c.seed)
    want = float64_forward(net, obs, cid)
    scale = max(1.0, float(want.abs().max()))
    with torch.no_grad():
        f32 = max_err(net(obs), want)
    emu = max_err(split_bf16_forward64(net, obs), want)
    return types.SimpleNamespace(case=c, net=net, obs=obs, std=std, want=want, scale=scale, bar=tol(c.kernel) * scale,
                                 f32_err=f32, emu_err=emu, control=f32 if c.kernel.build == "exact" else emu)
