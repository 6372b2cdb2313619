"""The comparison the wide learner GPU tests assert with (tests/wide_learner_check.py) must be able to fail: it is handed a float64
reference and perturbed copies of it, with the tolerances those tests use.  CPU only."""
import pytest
import torch

from tests import wide_learner_check as wl


@pytest.fixture(scope="module")
def reference():
    """Float64 outputs and parameter gradients of the high_level_game networks (19 -> 512-256-128 -> 6 | 1) on 37 rows; never modified."""
    spec = wl.CASES[0][1]
    nets = [wl.make_mlp(i, h, o, n).double() for n, (i, h, o) in enumerate(spec)]
    g = torch.Generator().manual_seed(5)
    x = torch.randn(37, 19, generator=g, dtype=torch.float64) * 2.0
    for n, net in enumerate(nets):
        wl.assert_both_elu_branches(net, x, f"net {n}")
    outs = [net(x) for net in nets]
    torch.autograd.backward(outs, [torch.randn(37, o, generator=g, dtype=torch.float64) / 37 for _, _, o in spec])
    grads = [p.grad for net in nets for p in net.parameters()]
    return wl.param_labels(nets), [o.detach() for o in outs], grads


def _check(labels, outs, grads, got_outs, got_grads, precision):
    wl.compare_all(["actor.output", "critic.output"], got_outs, outs, abs_tol=wl.OUT_TOL[precision])
    wl.compare_all(labels, got_grads, grads, rel=wl.GRAD_TOL[precision], abs_tol=wl.GRAD_ABS)


@pytest.mark.parametrize("precision", [0, 1])
def test_the_float32_rounding_of_the_reference_is_accepted(reference, precision):
    labels, outs, grads = reference
    _check(labels, outs, grads, [o.float() for o in outs], [g.float() for g in grads], precision)


@pytest.mark.parametrize("precision", [0, 1])
def test_one_element_of_the_smallest_weight_gradient_row_off_by_a_hundredth_of_the_max_is_rejected(reference, precision):
    labels, outs, grads = reference
    for k, g in enumerate(grads):
        if g.dim() != 2:
            continue
        bad = [x.float() for x in grads]
        row = int(g.abs().amax(dim=1).argmin())
        bad[k][row, g.shape[1] // 2] += 0.01 * float(g.abs().max())
        with pytest.raises(AssertionError, match=labels[k].replace(".", r"\.")):
            _check(labels, outs, grads, [o.float() for o in outs], bad, precision)


@pytest.mark.parametrize("precision", [0, 1])
def test_a_zeroed_bias_gradient_element_is_rejected(reference, precision):
    labels, outs, grads = reference
    for k, g in enumerate(grads):
        if g.dim() != 1:
            continue
        bad = [x.float() for x in grads]
        j = int(g.abs().argmax()) if g.numel() == 1 else int(g.abs().median(dim=0).indices)      # a typical element, not the largest
        bad[k][j] = 0.0
        with pytest.raises(AssertionError, match=labels[k].replace(".", r"\.")):
            _check(labels, outs, grads, [o.float() for o in outs], bad, precision)


@pytest.mark.parametrize("precision", [0, 1])
def test_two_swapped_output_columns_are_rejected(reference, precision):
    labels, outs, grads = reference
    bad = outs[0].float().clone()
    bad[:, [1, 4]] = bad[:, [4, 1]]
    with pytest.raises(AssertionError, match=r"actor\.output"):
        _check(labels, outs, grads, [bad, outs[1].float()], [g.float() for g in grads], precision)


@pytest.mark.parametrize("where", ["output", "weight", "bias"])
def test_a_nan_left_in_place_is_rejected(reference, where):
    labels, outs, grads = reference
    got_outs, got_grads = [o.float() for o in outs], [g.float() for g in grads]
    if where == "output":
        got_outs[1][36, 0] = float("nan")
    else:
        k = next(i for i, g in enumerate(grads) if g.dim() == (2 if where == "weight" else 1))
        got_grads[k].view(-1)[-1] = float("nan")
    with pytest.raises(AssertionError, match="non-finite"):
        _check(labels, outs, grads, got_outs, got_grads, 1)


def test_the_chain_rule_restated_for_the_cases():
    """Every case of the GPU test runs the per-layer forward GEMMs at precision 1; the registered rough shapes would not."""
    assert all(wl.takes_generic_forward(nets) for _, nets, _ in wl.CASES)
    assert not wl.takes_generic_forward([(235, wl.GAME_HIDDEN, 12), (235, wl.GAME_HIDDEN, 1)])
    assert not wl.takes_generic_forward([(169, wl.GAME_HIDDEN, 12), (169, wl.GAME_HIDDEN, 1)])
    assert wl.takes_generic_forward([(235, wl.GAME_HIDDEN, 12), (169, wl.GAME_HIDDEN, 1)])


def test_the_loss_input_check_rejects_degenerate_rows():
    ratio = torch.cat((torch.full((50,), 1.0), torch.full((50,), 1.5))).double()
    dv = torch.cat((torch.full((50,), 0.1), torch.full((50,), 0.3))).double()
    wl.assert_loss_inputs_not_degenerate(ratio, dv, 0.2)
    with pytest.raises(AssertionError, match="ratio inside"):
        wl.assert_loss_inputs_not_degenerate(torch.full((100,), 1.5).double(), dv, 0.2)
    with pytest.raises(AssertionError, match="value step"):
        wl.assert_loss_inputs_not_degenerate(ratio, torch.full((100,), 0.1).double(), 0.2)
    with pytest.raises(AssertionError, match="clip edge"):
        wl.assert_loss_inputs_not_degenerate(torch.cat((ratio[:-1], torch.tensor([1.2000001]).double())), dv, 0.2)
    g = torch.Generator().manual_seed(0)
    u = wl.spread(g, 4000, 0.6, (0.8, 1.2), 1.4, 0.02, "cpu")
    assert float(torch.minimum((u - 0.8).abs(), (u - 1.2).abs()).min()) >= 0.02 - 1e-12 and 0.58 <= float(u.min()) and float(u.max()) <= 1.42
