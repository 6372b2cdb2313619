"""Float64 restatement of the GRU cell of a recurrent policy's memory (gate order r, z, n of ``torch.nn.GRU``):

    r  = sigma(W_ir x + b_ir + W_hr h + b_hr)
    z  = sigma(W_iz x + b_iz + W_hz h + b_hz)
    n  = tanh(W_in x + b_in + r * (W_hn h + b_hn))
    h' = (1 - z) * n + z * h

from explicit arrays.  It shares no code with ``nn.GRU`` or the HIP kernels; tests/test_gru_check.py checks it against a ``.double()``
``nn.GRU`` on the CPU, and that its deliberately wrong variant (``b_hn`` outside the product with r) is far from it."""
import numpy as np


def _sigmoid(v):
    """1 / (1 + exp(-v)) written through tanh: no overflow at any |v| (exactly 0 / 1 once tanh saturates)."""
    return 0.5 * (1.0 + np.tanh(0.5 * v))


def gru_params64(rnn):
    """(w_ih, w_hh, b_ih, b_hh) of a one-layer ``nn.GRU`` as float64 arrays."""
    return tuple(p.detach().cpu().double().numpy() for p in (rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0))


def gru_step64(params, x, h, reset=None, b_hn_outside=False):
    """One step for every env: ``x`` [N, I], ``h`` [N, H]; rows with ``reset`` start from zeros.  Returns ``h'``.
    ``b_hn_outside``: the wrong cell that sums ``b_hn`` into the bias of n (the control of the tests' bar)."""
    w_ih, w_hh, b_ih, b_hh = params
    H = w_hh.shape[1]
    x, h = np.asarray(x, np.float64), np.asarray(h, np.float64)
    w_ir, w_iz, w_in = w_ih[:H], w_ih[H:2 * H], w_ih[2 * H:]
    w_hr, w_hz, w_hn = w_hh[:H], w_hh[H:2 * H], w_hh[2 * H:]
    b_ir, b_iz, b_in = b_ih[:H], b_ih[H:2 * H], b_ih[2 * H:]
    b_hr, b_hz, b_hn = b_hh[:H], b_hh[H:2 * H], b_hh[2 * H:]
    h_new = np.zeros_like(h)
    for row in range(x.shape[0]):
        hp = np.zeros(H) if (reset is not None and reset[row]) else h[row]
        r = _sigmoid(w_ir @ x[row] + b_ir + w_hr @ hp + b_hr)
        z = _sigmoid(w_iz @ x[row] + b_iz + w_hz @ hp + b_hz)
        if b_hn_outside:
            n = np.tanh(w_in @ x[row] + b_in + b_hn + r * (w_hn @ hp))
        else:
            n = np.tanh(w_in @ x[row] + b_in + r * (w_hn @ hp + b_hn))
        h_new[row] = (1.0 - z) * n + z * hp
    return h_new
