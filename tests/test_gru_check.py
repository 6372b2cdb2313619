"""The reference and the bar of tests/test_gpu_recurrent_gru.py, checked without a GPU: the float64 restatement ``tests/gru_ref.gru_step64``
equals a ``.double()`` ``nn.GRU``; the wrong cell that the bar has to catch -- ``b_hn`` summed into the bias of n, i.e. the LSTM cell's
layout with one gate dropped -- is more than 1000 bars away on every shape; and the GPU module's case table holds every shape the cell's
code paths need.  (The GPU module is parsed, not imported.)"""
import ast
import os

import numpy as np
import torch
import torch.nn as nn

from tests.gru_ref import gru_params64, gru_step64

REPO = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
GPU = "tests/test_gpu_recurrent_gru.py"
ROWS = 33


def _module():
    with open(os.path.join(REPO, GPU)) as f:
        return ast.parse(f.read())


def _constant(tree, name):
    return next(ast.literal_eval(n.value) for n in tree.body if isinstance(n, ast.Assign) and any(getattr(x, "id", None) == name for x in n.targets))


def _shapes():
    return sorted({(i, h) for i, h, _ in _constant(_module(), "CELL_CASES")})


def _inputs(I, H, seed):
    gen = torch.Generator().manual_seed(seed)
    x = (torch.rand(ROWS, I, generator=gen, dtype=torch.float64) * 2.0 - 1.0) * 3.0
    h = torch.rand(ROWS, H, generator=gen, dtype=torch.float64) * 2.0 - 1.0
    return x, h, torch.arange(ROWS) % 3 == 0


def test_the_restatement_equals_float64_torch_and_the_wrong_cell_is_a_thousand_bars_away():
    tol = _constant(_module(), "TOL")
    assert tol == 2e-5
    for I, H in _shapes():
        for gain in (1.0, 3.0):
            torch.manual_seed(I + H)
            rnn = nn.GRU(I, H).double()
            with torch.no_grad():
                rnn.weight_ih_l0.mul_(gain); rnn.weight_hh_l0.mul_(gain)
            x, h, reset = _inputs(I, H, I * 1000 + H)
            with torch.no_grad():
                want = rnn(x.unsqueeze(0), (h * (~reset).unsqueeze(1)).unsqueeze(0))[0][0].numpy()
            p = gru_params64(rnn)
            got = gru_step64(p, x.numpy(), h.numpy(), reset.numpy())
            assert np.abs(got - want).max() < 1e-12, (I, H, gain)
            assert np.abs(gru_step64(p, x.numpy(), h.numpy()) - rnn(x.unsqueeze(0), h.unsqueeze(0))[0][0].detach().numpy()).max() < 1e-12
            wrong = gru_step64(p, x.numpy(), h.numpy(), reset.numpy(), b_hn_outside=True)
            away = np.abs(wrong - want).max()
            assert away > 1000 * tol, (I, H, gain, away)


def test_the_case_table_holds_every_shape_the_cell_can_go_wrong_at():
    tree = _module()
    assert any(isinstance(n, ast.Assign) and any(getattr(x, "id", None) == "pytestmark" for x in n.targets) and "gpu" in ast.unparse(n.value)
               for n in tree.body), f"{GPU} is not marked gpu"
    cases = _constant(tree, "CELL_CASES")
    count = lambda values: {v: sum(v == w for w in values) for v in set(values)}
    ins, hids, rows = (count([c[k] for c in cases]) for k in range(3))
    assert set(ins) == {1, 3, 48, 235, 256} and set(hids) == {32, 64, 96, 160, 224, 256} and set(rows) == {1, 31, 32, 33, 65}
    assert all(v >= 2 for table in (ins, hids, rows) for v in table.values()), (ins, hids, rows)
    assert (256, 256) in {(i, h) for i, h, _ in cases}                               # the largest LDS block
    assert {(i + h) & 1 for i, h, _ in cases} == {0, 1}                               # the pad row of an odd K
    assert {i & 1 for i, _, _ in cases} == {0, 1}                                     # the x / h boundary inside one k-step, and between two
    # the other shapes the GPU tests name: different hidden sizes in one launch, the placement of the weight blocks
    text = open(os.path.join(REPO, GPU)).read()
    assert '"Ha,Hc", [(32, 256), (256, 64)]' in text and '"I,H", [(3, 32), (235, 64)]' in text
