"""-m gpu: the wide learner kernels at the shapes of ``dec_high_level_game`` with an asymmetric critic -- the actor on the agent's
observations, the critic on its privileged observations, each net with its own input tensor: (16 -> 4, 22 -> 1) for the prey and
(3 -> 2, 10 -> 1) for the predator.  22 inputs pad to 24 and 10 to 12 (layer 0's K is padded to a quad; the bias column follows), widths no
other case of tests/wide_learner_check.py has.  The check, the tolerances (``OUT_TOL``, ``GRAD_TOL``) and the mini-batch sizes (``MB_SMALL``)
are those of tests/test_gpu_wide_learner.py: float64 autograd on deep copies of the same modules, at both precisions."""
import pytest

from tests import wide_learner_check as wl
from tests.test_gpu_wide_learner import test_wide_kernels_match_float64_autograd_on_the_generic_path as _check_against_float64

pytestmark = pytest.mark.gpu

PRIVILEGED_CASES = [
    ("dec_prey_16_4_and_priv_22_1", [(16, wl.GAME_HIDDEN, 4), (22, wl.GAME_HIDDEN, 1)]),
    ("dec_pred_3_2_and_priv_10_1", [(3, wl.GAME_HIDDEN, 2), (10, wl.GAME_HIDDEN, 1)]),
]
_PARAMS = [pytest.param(nets, mb, gather, id=f"{cid}-mb{mb}") for cid, nets in PRIVILEGED_CASES for mb, gather in wl.MB_SMALL]


@pytest.mark.parametrize("precision", [1, 0])
@pytest.mark.parametrize("spec,mb,gather", _PARAMS)
def test_wide_kernels_match_float64_autograd_with_a_privileged_critic(spec, mb, gather, precision):
    assert (spec[1][0] + 3) // 4 * 4 in (24, 12) and spec[1][0] % 4 == 2            # the padded widths this file is about
    _check_against_float64(spec, False, mb, gather, precision)
