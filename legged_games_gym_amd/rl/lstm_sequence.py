"""The recurrence of a recurrent policy's PPO update on the device: ``DeviceLstmSequence`` stands in for ``nn.LSTM`` in
``Memory.forward``'s batch mode.  ``lg_lstm_seq_forward`` runs the padded trajectories through time in one launch and
``lg_lstm_seq_backward`` is back-propagation through time down to the gradient of the gate pre-activations (csrc/lg_lstm_seq.hip); the
weight gradients are three GEMMs on that in torch.  The torch module stays the owner of the parameters: every forward repacks them.
Numerics: the rollout cell's exact-f32 MFMA chain; tests compare against float64 autograd."""
import ctypes as C

import torch
import torch.nn as nn

from .. import capi


def sequence_unsupported_reason(rnn):
    """Why ``lg_lstm_seq_create`` does not take this ``nn.LSTM`` / ``nn.GRU``, or None."""
    if not isinstance(rnn, nn.LSTM):
        return f"{type(rnn).__name__} memory (the device sequence kernels are an LSTM's)"
    if rnn.num_layers != 1 or rnn.bidirectional or getattr(rnn, "proj_size", 0) or not rnn.bias:
        return f"{rnn.num_layers}-layer memory (the device sequence kernels run one plain layer)"
    if not capi.lstm_seq_supported(rnn.input_size, rnn.hidden_size):
        return (f"memory of {rnn.input_size} inputs and {rnn.hidden_size} units (the device sequence kernels take 1 .. {capi.LG_LSTM_SEQ_MAX_IN} "
                f"inputs and a multiple of 32 units up to {capi.LG_LSTM_SEQ_MAX_HIDDEN})")
    return None


def _check(lib, name, rc):
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc}): {lib.lg_lstm_seq_last_error().decode()}")


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


class _LstmSequenceFunction(torch.autograd.Function):
    """``h_out = LSTM(x; h0, c0)`` with gradients for the four parameter tensors only: observations and stored initial states take none."""

    @staticmethod
    def forward(ctx, seq, x, h0, c0, w_ih, w_hh, b_ih, b_hh):
        lib, (T, B, I), H = seq.lib, x.shape, seq.hidden
        rc = lib.lg_lstm_seq_load_device(seq.handle, w_ih.data_ptr(), w_hh.data_ptr(), b_ih.data_ptr(), b_hh.data_ptr(), _stream(x))
        _check(lib, "lg_lstm_seq_load_device", rc)
        h_out = torch.empty(T, B, H, device=x.device, dtype=torch.float32)
        needs = any(ctx.needs_input_grad[4:])
        ws = torch.empty(lib.lg_lstm_seq_workspace_floats(T, B, H), device=x.device, dtype=torch.float32) if needs else None
        rc = lib.lg_lstm_seq_forward(seq.handle, x.data_ptr(), x.stride(0) if T > 1 else B * I, h0.data_ptr(), c0.data_ptr(), h_out.data_ptr(),
                                     ws.data_ptr() if needs else None, T, B, _stream(x))
        _check(lib, "lg_lstm_seq_forward", rc)
        if needs:
            ctx.seq, ctx.ws = seq, ws
            ctx.save_for_backward(x, h0, c0, w_hh, h_out)
        return h_out

    @staticmethod
    def backward(ctx, dh_out):
        x, h0, c0, w_hh, h_out = ctx.saved_tensors
        seq, ws, lib = ctx.seq, ctx.ws, ctx.seq.lib
        if ws is None:
            raise RuntimeError("DeviceLstmSequence: backward ran twice through one forward (its workspace is overwritten in place)")
        ctx.ws = None
        (T, B, I), H = x.shape, seq.hidden
        dh_out = dh_out.contiguous().float()
        rc = lib.lg_lstm_seq_backward(seq.handle, w_hh.data_ptr(), dh_out.data_ptr(), c0.data_ptr(), ws.data_ptr(), T, B, _stream(x))
        _check(lib, "lg_lstm_seq_backward", rc)
        dG = ws[:T * B * 4 * H].view(T * B, 4 * H)
        h_prev = torch.cat((h0.unsqueeze(0), h_out[:-1]), 0).reshape(T * B, H)
        dGt = dG.t()
        dw_ih = dGt @ x.reshape(T * B, I)
        dw_hh = dGt @ h_prev
        db = dG.sum(0)
        return None, None, None, None, dw_ih, dw_hh, db, db.clone()


class DeviceLstmSequence:
    """One ``lg_lstm_seq`` handle over a one-layer ``nn.LSTM``; callable as ``(input [T, B, I], (h0, c0) [1, B, H]) -> out [T, B, H]``,
    which is ``rnn(input, (h0, c0))[0]`` with the recurrence on the device kernels, forward and backward."""

    def __init__(self, rnn, device):
        why = sequence_unsupported_reason(rnn)
        if why is not None:
            raise ValueError(f"no device LSTM sequence kernels for a {why}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("the device LSTM sequence kernels need a CUDA device")
        self.lib, self.rnn = capi.load_lstm_seq_library(), rnn
        self.num_in, self.hidden = rnn.input_size, rnn.hidden_size
        self.handle = C.c_void_p()
        rc = self.lib.lg_lstm_seq_create(self.num_in, self.hidden, self.device.index or 0, C.byref(self.handle))
        _check(self.lib, "lg_lstm_seq_create", rc)

    @staticmethod
    def _plain(t):
        """float32, rows contiguous; a slice along dimension 1 of a wider [T, B', F] tensor is passed as it is (a step stride)."""
        if t.dtype != torch.float32:
            t = t.float()
        if t.dim() == 3 and (t.stride(2) != 1 or t.stride(1) != t.shape[2] or t.stride(0) < t.shape[1] * t.shape[2]):
            t = t.contiguous()
        return t

    def __call__(self, input, hidden_states):
        h0, c0 = hidden_states
        r = self.rnn
        params = (r.weight_ih_l0, r.weight_hh_l0, r.bias_ih_l0, r.bias_hh_l0)
        for p in params:
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise ValueError("DeviceLstmSequence needs contiguous float32 CUDA parameters")
        if input.dim() != 3 or input.shape[2] != self.num_in or not input.is_cuda:
            raise ValueError(f"DeviceLstmSequence: input must be a CUDA tensor [T, B, {self.num_in}], got {tuple(input.shape)} on {input.device}")
        B = input.shape[1]
        state = lambda s: s.detach().reshape(B, self.hidden).float().contiguous()
        return _LstmSequenceFunction.apply(self, self._plain(input.detach()), state(h0), state(c0), *params)

    def __deepcopy__(self, memo):
        """A deep copy of the module that holds this has an ``nn.LSTM`` of its own and no handle: it is back on torch (``sequence = None``)."""
        return None

    def __del__(self):
        try:
            if self.handle:
                self.lib.lg_lstm_seq_destroy(self.handle)
                self.handle = C.c_void_p()
        except Exception:
            pass
