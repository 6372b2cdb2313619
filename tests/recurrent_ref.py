"""Float64 restatements of the recurrent policy's two device stages: a one-layer LSTM with explicit gate arithmetic per env and step
(gate order i, f, g, o of ``torch.nn.LSTM``) and the actor MLP behind it (Linear / ELU x 3 / Linear) from explicit arrays.  They share no
code with ``nn.LSTM``, ``nn.Sequential`` or the HIP kernels; tests/test_recurrent_policy.py checks both against ``.double()`` copies of
the torch modules on the CPU."""
import numpy as np


def _sigmoid(v):
    """1 / (1 + exp(-v)) written through tanh: no overflow at any |v| (exactly 0 / 1 once tanh saturates)."""
    return 0.5 * (1.0 + np.tanh(0.5 * v))


def lstm_params64(rnn):
    """(w_ih, w_hh, b_ih, b_hh) of a one-layer ``nn.LSTM`` as float64 arrays."""
    return tuple(p.detach().cpu().double().numpy() for p in (rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0))


def lstm_step64(params, x, h, c, reset=None):
    """One step for every env: ``x`` [N, I], ``h`` / ``c`` [N, H]; rows with ``reset`` start from zeros.  Returns ``(h', c')``."""
    w_ih, w_hh, b_ih, b_hh = params
    H = w_hh.shape[1]
    x, h, c = np.asarray(x, np.float64), np.asarray(h, np.float64), np.asarray(c, np.float64)
    h_new, c_new = np.zeros_like(h), np.zeros_like(c)
    for n in range(x.shape[0]):
        hn, cn = (np.zeros(H), np.zeros(H)) if (reset is not None and reset[n]) else (h[n], c[n])
        for u in range(H):
            pre = [b_ih[g * H + u] + b_hh[g * H + u] + np.dot(w_ih[g * H + u], x[n]) + np.dot(w_hh[g * H + u], hn) for g in range(4)]
            i, f, g, o = _sigmoid(pre[0]), _sigmoid(pre[1]), np.tanh(pre[2]), _sigmoid(pre[3])
            c_new[n, u] = f * cn[u] + i * g
            h_new[n, u] = o * np.tanh(c_new[n, u])
    return h_new, c_new


SATURATING = (30.0, 100.0, 1e4, -30.0, -100.0, -1e4, 0.0, 0.0)


def saturating_bias(H):
    """float64 [4 H]: ``SATURATING[(u + 3 g) % 8]`` at row ``g H + u``, to be added to ``bias_ih_l0``: every gate meets every magnitude,
    each in a different unit, and the four gates of one unit meet four different ones."""
    return np.array([SATURATING[(u + 3 * g) % 8] for g in range(4) for u in range(H)])


def actor_params64(layers):
    """(weights, biases) of the ``nn.Linear`` modules in ``layers`` (an ``nn.Sequential`` or a list) as lists of float64 arrays."""
    lin = [m for m in layers if hasattr(m, "weight") and hasattr(m, "in_features")]
    return [m.weight.detach().cpu().double().numpy() for m in lin], [m.bias.detach().cpu().double().numpy() for m in lin]


def actor_forward64(weights, biases, h):
    """The actor MLP on ``h`` [N, dims[0]]: ``weights[l]`` is [out_l, in_l] (``nn.Linear``'s layout), ELU (alpha 1) after every layer but
    the last.  Every output is one explicit float64 dot product.  Returns the means [N, actions]."""
    x = np.asarray(h, np.float64)
    last = len(weights) - 1
    for l, (w, b) in enumerate(zip(weights, biases)):
        w, b = np.asarray(w, np.float64), np.asarray(b, np.float64)
        assert w.shape == (b.shape[0], x.shape[1]), (l, w.shape, b.shape, x.shape)
        y = np.empty((x.shape[0], w.shape[0]))
        for n in range(x.shape[0]):
            for o in range(w.shape[0]):
                v = b[o] + np.dot(w[o], x[n])
                y[n, o] = v if (l == last or v > 0.0) else np.expm1(v)
        x = y
    return x
