"""Shared pieces of tests/test_gpu_chain_forward_edges.py (GPU) and tests/test_chain_check.py (CPU): the case table of the chain
forward kernel (csrc/lg_policy.h: k_mlp_chain_fwd64<15>, <11>, k_chain_pack), the inputs and the float64 reference of every case, and
a restatement of the kernel's arithmetic in torch that can be told to make one of the errors the GPU tests are there to find.
Nothing here touches the device library, so the table and the bars are tested without a GPU."""
import collections
import copy
import functools

import torch

from tests import wide_learner_check as wl

HIDDEN = wl.GAME_HIDDEN                      # the only hidden widths the chain is compiled for
ROWS_PER_WG, HALF = 64, 32                   # rows of a workgroup; of one of its two MFMA row halves
K0S_OF = {11: range(161, 177), 15: range(225, 241)}      # layer-0 k-steps -> the input widths the host rule accepts
PRECISION = 1                                # lg_mlp_wide_set_precision: the chain runs at 1 only
OUT_BAR, GRAD_BAR, GRAD_ABS = wl.OUT_TOL[PRECISION], wl.GRAD_TOL[PRECISION], wl.GRAD_ABS

Case = collections.namedtuple("Case", "id nets shared mb gathered why")


def _c(cid, nets, shared, mb, gathered, why):
    return Case(cid, tuple(nets), shared, mb, gathered, why)


def _pair(w, a=12, c=1):
    return [(w, a), (w, c)]


# (id, [(inputs, outputs) per net], both nets read one input tensor, mini-batch rows, gathered through a row list) -- each the smallest
# at which its mechanism exists.  The last k-step of layer 0 is staged as two lane halves h of two quads each (columns
# 16 ks + 8 h + 0..3 | + 4..7) against ldx = round-up(inputs, 4): what is live there is written beside each width.
CASES = [
    # ---- input widths, K0S = 15 (last k-step: columns 224 .. 239): actor 12 + critic 1 on one table, 37 rows (a second row half of 5)
    _c("w225", _pair(225), True, 37, True, "first width of the range: one quad live (h = 0 only), 3 of its 4 columns padding"),
    _c("w229", _pair(229), True, 37, False, "both quads of h = 0 live, none of h = 1; the second quad has one real column"),
    _c("w232", _pair(232), True, 37, True, "h = 0 full, h = 1 empty, no padding column (inputs a multiple of 4 and of 8)"),
    _c("w236", _pair(236), True, 37, False, "three quads live, no padding column"),
    _c("w237", _pair(237), True, 37, True, "four quads live, three padding columns in the last"),
    _c("w240", _pair(240), True, 37, True, "last width of the range: every column of the last k-step real"),
    # ---- K0S = 11 (columns 160 .. 175)
    _c("w161", _pair(161), True, 37, True, "first width of the range: one quad live"),
    _c("w165", _pair(165), True, 37, False, "both quads of h = 0 live, none of h = 1"),
    _c("w168", _pair(168), True, 37, True, "h = 0 full, h = 1 empty, no padding column"),
    _c("w172", _pair(172), True, 37, False, "three quads live, no padding column"),
    _c("w173", _pair(173), True, 37, True, "four quads live, three padding columns"),
    _c("w176", _pair(176), True, 37, True, "last width of the range"),
    # ---- output counts x mb = 33 (a second row half with one live row): a = 8 ii + 4 h + r < out_dim, biases by (ii = 0) and by2 (ii = 1)
    _c("o2_o4_k15", [(235, 2), (235, 4)], True, 33, True, "inside the first h group | exactly the h = 0 group"),
    _c("o5_o8_k15", [(235, 5), (235, 8)], True, 33, False, "one action into h = 1 | exactly ii = 0: by2 never used"),
    _c("o9_o13_k15", [(235, 9), (235, 13)], True, 33, True, "one action of by2 | one action into h = 1 of by2"),
    _c("o16_o1_k15", [(235, 16), (235, 1)], True, 33, True, "every lane writes | one lane group writes"),
    _c("o2_o4_k11", [(169, 2), (169, 4)], True, 33, False, "as above on <11>"),
    _c("o5_o8_k11", [(169, 5), (169, 8)], True, 33, True, "as above on <11>"),
    _c("o9_o13_k11", [(169, 9), (169, 13)], True, 33, True, "as above on <11>"),
    _c("o16_o12_k11", [(169, 16), (169, 12)], True, 33, True, "as above on <11>; 12 = by2's h = 0 group exactly"),
    # ---- a single net (grid.y = 1, the second descriptor mirrors the first) x the ends of the width ranges
    _c("single_225_critic", [(225, 1)], False, 37, True, "single net, critic shape, first width of <15>"),
    _c("single_240_actor", [(240, 5)], False, 37, False, "single net, actor shape, last width of <15>"),
    _c("single_161_actor", [(161, 16)], False, 37, True, "single net, actor shape, first width of <11>"),
    _c("single_176_critic", [(176, 1)], False, 37, False, "single net, critic shape, last width of <11>"),
    # ---- two nets on separate tensors: per-net x / ldx / workspace slice
    _c("sep_235_235", [(235, 12), (235, 1)], False, 37, True, "separate tensors of one width"),
    _c("sep_235_229", [(235, 12), (229, 1)], False, 37, True, "same K0S, ldx 236 against 232"),
    _c("sep_169_169", [(169, 12), (169, 1)], False, 37, True, "separate tensors of one width"),
    _c("sep_169_165", [(169, 12), (165, 1)], False, 37, False, "same K0S, ldx 172 against 168"),
    # ---- rows: a workgroup takes 64 in two halves of 32, a dead row is clamped to mb - 1 (33 is above)
    _c("mb1_k15", _pair(235), True, 1, True, "one live row: 63 clamped onto it; the row list is the table's last row"),
    _c("mb31_k15", _pair(235), True, 31, False, "first half one row short, second half dead"),
    _c("mb32_k15", _pair(235), True, 32, True, "first half full, second half dead"),
    _c("mb63_k15", _pair(235), True, 63, False, "second half one row short"),
    _c("mb64_k15", _pair(235), True, 64, True, "one full workgroup, no dead row"),
    _c("mb65_k15", _pair(235), True, 65, True, "anymal_c_rough's nets (three quads live, one padding column): a second workgroup with one live row"),
    _c("mb1025_k15", _pair(235), True, 1025, True, "17 workgroups: every wv, r1, r2, every r0; the last with one live row"),
    _c("mb1_k11", _pair(169), True, 1, False, "one live row, rows = None"),
    _c("mb31_k11", _pair(169), True, 31, True, "as above on <11>"),
    _c("mb32_k11", _pair(169), True, 32, False, "as above on <11>"),
    _c("mb63_k11", _pair(169), True, 63, True, "as above on <11>"),
    _c("mb64_k11", _pair(169), True, 64, False, "as above on <11>"),
    _c("mb65_k11", _pair(169), True, 65, True, "cassie's nets (three quads live, three padding columns): a second workgroup with one live row"),
    _c("mb1025_k11", _pair(169), True, 1025, False, "17 workgroups on <11>, rows = None"),
]
BY_ID = {c.id: c for c in CASES}
BASE = {15: "mb65_k15", 11: "mb65_k11"}              # the base case of each kernel: what the single-case tests run
ROW_PROBE_CASES = ("o9_o13_k15", "o16_o12_k11", "mb65_k15", "mb65_k11", "mb1025_k15", "mb1025_k11")     # mb = 33, 65 and 1025, both kernels
ROW_PROBES = (0, 31, 32, 63, 64)             # ... and mb - 1: both sides of the half and of the workgroup boundary
REPEAT = "mb1025_k15"

WIDTHS = {11: (161, 165, 168, 169, 172, 173, 176), 15: (225, 229, 232, 235, 236, 237, 240)}
OUTPUTS = (1, 2, 4, 5, 8, 9, 12, 13, 16)
NEW_OUTPUTS = tuple(o for o in OUTPUTS if o not in (1, 12))      # 12 and 1 are what the suite ran before this table
MBS = (1, 31, 32, 33, 63, 64, 65, 1025)


def k0s(width):
    return (width + 15) // 16


def case_k0s(case):
    return k0s(case.nets[0][0])


def spec(case):
    """The case's nets as wide_learner_check writes them: (inputs, hidden widths, outputs)."""
    return [(i, HIDDEN, o) for i, o in case.nets]


def takes_the_chain(nets):
    """The host rule of lg_mlp_wide_forward at precision 1 -- wl.takes_generic_forward, not a second copy of it."""
    return not wl.takes_generic_forward([(i, HIDDEN, o) for i, o in nets])


def staging(width):
    """What the last k-step of layer 0 holds for ``width`` inputs: (live quads of lane half 0, of lane half 1, padding columns in the
    last live quad) -- the two branches ``k0 + 4 <= ldx`` and ``k0 + 8 <= ldx`` of the kernel's staging, k0 = 16 ks + 8 h."""
    ldx, ks = (width + 3) & ~3, k0s(width) - 1
    quads = [sum(1 for q in (4, 8) if 16 * ks + 8 * h + q <= ldx) for h in (0, 1)]
    return quads[0], quads[1], ldx - width


def workgroup_walk(mb, k):
    """The per-workgroup rotations of k_mlp_chain_fwd64<k> over the grid of ``mb`` rows: the sets of wv (per wave), r0, r1, r2 taken, the
    number of workgroups and the live rows of the last one."""
    blocks = (mb + ROWS_PER_WG - 1) // ROWS_PER_WG
    wv = {w: {(w + b) & 7 for b in range(blocks)} for w in range(8)}
    r0, r1, r2 = ({(5 * b) % k for b in range(blocks)}, {(5 * b) & 15 for b in range(blocks)}, {(3 * b) & 15 for b in range(blocks)})
    return wv, r0, r1, r2, blocks, mb - ROWS_PER_WG * (blocks - 1)


def assert_1025_rows_walk_every_rotation():
    """mb = 1025 = 16 * 64 + 1: 17 workgroups.  wv = (wave + blk) & 7 takes all 8 values on every wave within blk 0 .. 7; r1 = 5 blk & 15
    and r2 = 3 blk & 15 (5 and 3 odd) take all 16 within blk 0 .. 15; r0 = 5 blk % K0S takes all 11 values within blk 0 .. 10 on <11>
    and the three values {0, 5, 10} it can ever take on <15> (gcd(5, 15) = 5) within blk 0 .. 2.  Workgroup 16 has one live row."""
    for k in (11, 15):
        wv, r0, r1, r2, blocks, last = workgroup_walk(1025, k)
        assert blocks == 17 and last == 1
        assert all(v == set(range(8)) for v in wv.values()) and r1 == set(range(16)) and r2 == set(range(16))
        assert r0 == {(5 * b) % k for b in range(100000)} and len(r0) == (11 if k == 11 else 3)
        short = workgroup_walk(1024 - 64, k)                     # 15 workgroups are one too few for r1 / r2
        assert len(short[2]) == 15 and len(short[3]) == 15


# ------------------------------------------------------------------ inputs and the float64 reference, once per case
Inputs = collections.namedtuple("Inputs", "case nets xs rows table_rows")
Reference = collections.namedtuple("Reference", "inputs refs xb want_out d_out want_grads f32_out_err f32_grad_err")


def table_rows(case):
    return 2 * case.mb + 7 if case.gathered else case.mb


def row_list(mb, R, g):
    """A row list with the first and the last row of the table and, from 8 rows on, two repeated rows (one repeat next to its original,
    the table's last row a second time half a mini-batch away); a single row is the table's last."""
    rows = torch.randint(0, R, (mb,), generator=g)
    rows[-1] = R - 1
    if mb >= 2:
        rows[0] = 0
    if mb >= 8:
        rows[2] = rows[1]
        rows[mb // 2 + 1] = R - 1
    return rows


@functools.lru_cache(maxsize=None)
def inputs(cid, seed=5):
    """Networks (torch default initialisation, seeds 0 and 1 as the wide learner tests), input tables (randn * 2: both ELU branches in
    every layer) and row list of a case, on the CPU: the GPU test moves copies of exactly these to the device."""
    case = BY_ID[cid]
    nets = [wl.make_mlp(i, HIDDEN, o, n) for n, (i, o) in enumerate(case.nets)]
    g = torch.Generator().manual_seed(seed)
    R = table_rows(case)
    xs = [torch.randn(R, case.nets[0][0], generator=g) * 2.0]
    for i, _ in case.nets[1:]:
        xs.append(xs[0] if case.shared else torch.randn(R, i, generator=g) * 2.0)
    rows = row_list(case.mb, R, g) if case.gathered else None
    return Inputs(case, nets, xs, rows, R)


def batch(inp):
    """The mini-batch rows of every net's table."""
    return [(x[inp.rows] if inp.rows is not None else x[:inp.case.mb]) for x in inp.xs]


@functools.lru_cache(maxsize=None)
def reference(cid):
    """float64 outputs and float64 autograd gradients (for d_out = randn / mb) of a case on deep copies of its modules, and the error of
    torch's own float32 forward / autograd on the same modules, for scale.  Shared by every test of the case; treat as read-only."""
    inp = inputs(cid)
    mb = inp.case.mb
    xb = batch(inp)
    refs = [wl.float64_copy(n) for n in inp.nets]
    f32 = [copy.deepcopy(n) for n in inp.nets]
    g = torch.Generator().manual_seed(11)
    d_out = [torch.randn(mb, o, generator=g) / mb for _, o in inp.case.nets]
    want_out = [r(x.double()) for r, x in zip(refs, xb)]
    f32_out = [n(x) for n, x in zip(f32, xb)]
    torch.autograd.backward(want_out, [d.double() for d in d_out])
    torch.autograd.backward(f32_out, d_out)
    want = [p.grad.clone() for r in refs for p in r.parameters()]
    f32_grads = [p.grad for n in f32 for p in n.parameters()]
    for r in refs:
        r.zero_grad(set_to_none=True)
    return Reference(inp, refs, xb, [w.detach() for w in want_out], d_out, want,
                     wl.max_error(f32_out, want_out, False), wl.max_error(f32_grads, want, True))


def one_row_grads(ref, r, d_row):
    """float64 autograd of every parameter for a d_out that is ``d_row[n]`` in row ``r`` and zero elsewhere: only row ``r`` of the
    mini-batch takes part, so the reference runs that one row."""
    outs = [net(x[r:r + 1].double()) for net, x in zip(ref.refs, ref.xb)]
    grads = torch.autograd.grad(outs, [p for net in ref.refs for p in net.parameters()], [d.double().reshape(1, -1) for d in d_row])
    return list(grads)


# ------------------------------------------------------------------ the kernel's arithmetic, restated
LOG2E = 1.442695041                          # the literal of elu1() in csrc/lg_policy.h
PLANTS = ("lo_dropped_0", "lo_dropped_1", "lo_dropped_2", "lo_dropped_3", "last_input_column", "last_hidden_column", "by2_bias",
          "rows_31_32_exchanged", "dead_row_clamp_to_0")


def split(v):
    """hi = bf16(v), lo = bf16(v - hi), both back in float32 (split8 / pack_wide_body; round to nearest even, as the hardware converts)."""
    hi = v.bfloat16().float()
    return hi, (v - hi).bfloat16().float()


def plant_applies(plant, net, mb):
    """Whether a planted error changes anything for a net of ``net`` = (inputs, outputs) at ``mb`` rows."""
    if plant == "by2_bias":
        return net[1] > 8
    if plant == "rows_31_32_exchanged":
        return mb > HALF
    if plant == "dead_row_clamp_to_0":
        return mb > 1 and mb % ROWS_PER_WG != 0
    return plant in PLANTS


def chain_forward_restated(net, x, plant=None):
    """What k_mlp_chain_fwd64 computes for the float32 module ``net`` on the float32 rows ``x``, in torch on the CPU: every operand split
    into bf16 hi + lo, products hi.hi + hi.lo + lo.hi accumulated in float32 (the MFMA's products of two bf16 are exact in float32),
    bias added in float32, ELU as exp2(1.442695041 z) - 1 below 0; the layer-0 weight columns at or past the input width are zero, so
    they are simply absent here.  ``plant`` makes one error a wrong kernel could make (PLANTS)."""
    assert plant is None or plant in PLANTS, plant
    assert x.dtype == torch.float32
    layers = [m for m in net if isinstance(m, torch.nn.Linear)]
    h = x
    with torch.no_grad():
        for l, m in enumerate(layers):
            w, b = m.weight.detach(), m.bias.detach().clone()
            if (plant == "last_input_column" and l == 0) or (plant == "last_hidden_column" and l == 3):
                h = h.clone()
                h[:, -1] = 0.0
            hh, hl = split(h)
            if plant == f"lo_dropped_{l}":
                hl = torch.zeros_like(hl)
            wh, wlo = split(w)
            z = hh @ wlo.t() + hl @ wh.t() + hh @ wh.t()          # small terms first, as the kernel issues them
            if plant == "by2_bias" and l == 3:
                b[8:] = 0.0
            z = z + b
            h = torch.where(z > 0, z, torch.exp2(LOG2E * z) - 1.0) if l < 3 else z
        out = h
        mb = out.shape[0]
        if plant == "rows_31_32_exchanged" and mb > HALF:                             # the last row of half 0 and the first of half 1
            out = out.clone()
            out[[HALF - 1, HALF]] = out[[HALF, HALF - 1]]
        if plant == "dead_row_clamp_to_0" and mb > 1 and mb % ROWS_PER_WG != 0:      # the dead rows of the last workgroup compute row 0 and
            out = out.clone()                                                         # store it where they were clamped to
            out[mb - 1] = out[0]
    assert out.dtype == torch.float32
    return out


def bars_out(got, want, bar=OUT_BAR):
    """Largest |got - want| over lists of tensors as a multiple of the absolute output bar."""
    return max(float((g.double() - w.double()).abs().max()) for g, w in zip(got, want)) / bar


def restated_outputs(cid, plant=None):
    ref = reference(cid)
    return [chain_forward_restated(n, x, plant) for n, x in zip(ref.inputs.nets, ref.xb)]


# ------------------------------------------------------------------ the host rule
def assert_the_host_rule():
    """Every case takes the chain; the widths next to the two ranges and 17 outputs do not; nor do two nets of different K0S."""
    for c in CASES:
        assert takes_the_chain(c.nets), c.id
        assert all(i in K0S_OF[case_k0s(c)] for i, _ in c.nets) and all(1 <= o <= 16 for _, o in c.nets), c.id
    for w in (160, 177, 224, 241):
        assert not takes_the_chain([(w, 12)]) and not takes_the_chain(_pair(w)), w
    for w in (161, 176, 225, 240):
        assert takes_the_chain([(w, 16)]) and not takes_the_chain([(w, 17)]), w
    assert not takes_the_chain([(235, 12), (169, 1)])
