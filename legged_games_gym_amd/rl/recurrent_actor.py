"""Rollout-time recurrent policy on the matrix cores: both LSTM memories of an ``ActorCriticRecurrent`` advance in ONE launch
(``lg_lstm_step``, csrc/lg_recurrent.hip), then the actor MLP runs on the actor memory's ``h`` in ``lg_lstm_actor_act`` with the Philox
exploration noise of ``lg_policy_act`` (whose kernels exist for the tasks' observation widths only, not for a memory's 64 or 256 units).  The torch module stays the owner of the parameters; ``sync_device()`` repacks them on the device.
Numerics: exact-f32 MFMA (k-ordered fmaf chains); tests compare against a float64 restatement."""
import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from .. import capi


def lstm_unsupported_reason(rnn, wide=False):
    """Why ``lg_lstm_create`` (``wide``: ``lg_lstm_wide_create``) does not take this ``nn.LSTM`` / ``nn.GRU``, or None."""
    if not isinstance(rnn, nn.LSTM):
        return f"{type(rnn).__name__} memory (the device cell is an LSTM)"
    if rnn.num_layers != 1 or rnn.bidirectional or getattr(rnn, "proj_size", 0) or not rnn.bias:
        return f"{rnn.num_layers}-layer memory (the device cell is one plain layer)"
    if wide:
        if not capi.lstm_wide_supported(rnn.input_size, rnn.hidden_size):
            return (f"memory of {rnn.input_size} inputs and {rnn.hidden_size} units (the wide device cell takes 1 .. {capi.LG_LSTM_WIDE_MAX_IN} "
                    f"inputs and a multiple of 32 units up to {capi.LG_LSTM_WIDE_MAX_HIDDEN})")
        return None
    if not capi.lstm_supported(rnn.input_size, rnn.hidden_size):
        return (f"memory of {rnn.input_size} inputs and {rnn.hidden_size} units (the device cell takes 1 .. {capi.LG_LSTM_MAX_IN} inputs and "
                f"a multiple of 32 units up to {capi.LG_LSTM_MAX_HIDDEN})")
    return None


def gru_unsupported_reason(rnn):
    """Why ``lg_gru_create`` (the runner key ``device_gru``) does not take this ``nn.GRU`` / ``nn.LSTM``, or None."""
    if not isinstance(rnn, nn.GRU):
        return f"{type(rnn).__name__} memory (the device GRU cell is a GRU)"
    if rnn.num_layers != 1 or rnn.bidirectional or not rnn.bias:
        return f"{rnn.num_layers}-layer memory (the device GRU cell is one plain layer)"
    if not capi.gru_supported(rnn.input_size, rnn.hidden_size):
        return (f"memory of {rnn.input_size} inputs and {rnn.hidden_size} units (the device GRU cell takes 1 .. {capi.LG_GRU_MAX_IN} inputs and "
                f"a multiple of 32 units up to {capi.LG_GRU_MAX_HIDDEN})")
    return None


def device_gru_would_help(rnn):
    """Whether the key ``device_gru`` turns a refusal of this memory into an acceptance (the fall-back messages then name it)."""
    return lstm_unsupported_reason(rnn) is not None and gru_unsupported_reason(rnn) is None


def wide_memory_would_help(rnn):
    """Whether the key ``wide_memory`` turns a refusal of this memory into an acceptance (the fall-back messages then name it)."""
    return lstm_unsupported_reason(rnn) is not None and lstm_unsupported_reason(rnn, wide=True) is None


# kind of a cell memory -> (its record in capi.LIBRARIES, the prefix of its entry points, the library's last-error entry point, its name in messages)
MEMORY_KINDS = {
    "lstm": ("main", "lg_lstm", "lg_last_error", "LSTM"),
    "lstm_wide": ("lstm_wide", "lg_lstm_wide", "lg_lstm_wide_last_error", "LSTM"),       # up to 512 units; the signatures of lg_lstm_*
    "gru": ("gru", "lg_gru", "lg_gru_last_error", "GRU"),                                # one state tensor: lg_gru_step has its own signature
}


class DeviceMemory:
    """One cell-memory handle (``lg_lstm``, ``lg_lstm_wide`` or ``lg_gru``, by ``kind``) over a one-layer ``nn.LSTM`` / ``nn.GRU``: create from
    the host copies of the parameters, repack from the CUDA parameters, destroy.  The three libraries' entry points have the same
    signatures but for ``*_step``."""

    def __init__(self, rnn, device, kind):
        record, self._pre, last_error, cell = MEMORY_KINDS[kind]
        why = gru_unsupported_reason(rnn) if kind == "gru" else lstm_unsupported_reason(rnn, kind == "lstm_wide")
        if why is not None:
            raise ValueError(f"no device {cell} cell for a {why}")
        self.kind, self.wide, self.gru = kind, kind == "lstm_wide", kind == "gru"
        self.lib, self.rnn, self.device = capi.load(record), rnn, torch.device(device)
        self._last_error = getattr(self.lib, last_error)
        self.num_in, self.hidden = rnn.input_size, rnn.hidden_size
        self.handle = C.c_void_p()
        host = [np.ascontiguousarray(p.detach().float().cpu().numpy()) for p in self._params()]
        self._call("_create", self.num_in, self.hidden, *[a.ctypes.data for a in host], self.device.index or 0, C.byref(self.handle))

    def _call(self, entry, *args, lib=None):
        """Entry point ``<prefix><entry>`` of ``lib`` (default: the handle's library); a RuntimeError with the library's message on failure."""
        rc = getattr(lib or self.lib, self._pre + entry)(*args)
        if rc != 0:
            raise RuntimeError(f"{self._pre}{entry} failed ({rc}): {self._last_error().decode()}")

    def _params(self):
        r = self.rnn
        return r.weight_ih_l0, r.weight_hh_l0, r.bias_ih_l0, r.bias_hh_l0

    def load_device(self):
        """Repack from the module's CUDA parameters (``*_load_device``): one launch on the current stream, no host copy."""
        ps = self._params()
        for p in ps:
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise ValueError(f"{type(self).__name__}.load_device needs contiguous float32 CUDA parameters")
        self._call("_load_device", self.handle, *[p.data_ptr() for p in ps], torch.cuda.current_stream(self.device).cuda_stream)

    def __del__(self):
        try:
            if self.handle:
                getattr(self.lib, self._pre + "_destroy")(self.handle)
                self.handle = C.c_void_p()
        except Exception:
            pass


class DeviceLstm(DeviceMemory):
    """One ``lg_lstm`` handle over a one-layer ``nn.LSTM``; with ``wide`` one ``lg_lstm_wide`` handle of liblegged_lstm_wide.so (up to 512 units)."""

    def __init__(self, rnn, device, wide=False):
        super().__init__(rnn, device, "lstm_wide" if wide else "lstm")


class DeviceGru(DeviceMemory):
    """One ``lg_gru`` handle of liblegged_gru.so over a one-layer ``nn.GRU``."""

    def __init__(self, rnn, device):
        super().__init__(rnn, device, "gru")


def gru_step(lib, gru_a, gru_c, x_a, x_c, reset, h_in_a, h_out_a, h_in_c, h_out_c, num_envs, stream):
    """``lg_gru_step`` on tensors; a role is absent when its ``DeviceGru`` is None.  ``lib`` is liblegged_gru.so."""
    p = lambda t, present: None if (t is None or not present) else t.data_ptr()
    a, c = gru_a is not None, gru_c is not None
    (gru_a if a else gru_c)._call("_step", gru_a.handle if a else None, gru_c.handle if c else None, p(x_a, a), p(x_c, c), p(reset, True),
                                  p(h_in_a, a), p(h_out_a, a), p(h_in_c, c), p(h_out_c, c), int(num_envs), stream, lib=lib)


def lstm_step(lib, lstm_a, lstm_c, x_a, x_c, reset, state_in_a, state_out_a, state_in_c, state_out_c, num_envs, stream):
    """``lg_lstm_step`` on tensors; a role is absent when its ``DeviceLstm`` is None.  ``state_*`` are ``(h, c)`` pairs.  ``lib`` is the
    library of the handles: with ``wide`` memories (liblegged_lstm_wide.so) the launch is ``lg_lstm_wide_step``, by the handles' kind."""
    p = lambda t: None if t is None else t.data_ptr()
    ha, ca = state_in_a if lstm_a is not None else (None, None)
    hoa, coa = state_out_a if lstm_a is not None else (None, None)
    hc, cc = state_in_c if lstm_c is not None else (None, None)
    hoc, coc = state_out_c if lstm_c is not None else (None, None)
    (lstm_a if lstm_a is not None else lstm_c)._call(
        "_step", lstm_a.handle if lstm_a is not None else None, lstm_c.handle if lstm_c is not None else None,
        p(x_a) if lstm_a is not None else None, p(x_c) if lstm_c is not None else None, p(reset),
        p(ha), p(ca), p(hoa), p(coa), p(hc), p(cc), p(hoc), p(coc), int(num_envs), stream, lib=lib)


class DeviceLstmActor:
    """One ``lg_lstm_actor`` handle over ``actor_critic.actor`` (Linear / ELU x 3 / Linear) and ``actor_critic.std``; the step bookkeeping
    of ``FusedActor``: the env's device step counter when given, a host count otherwise.  With ``wide`` the handle is an
    ``lg_lstm_wide_actor`` of liblegged_lstm_wide.so (an input width up to 512)."""

    def __init__(self, actor_critic, device, seed=1, step_counter=None, wide=False):
        self.wide = bool(wide)
        self.lib, self.ac, self.device = (capi.load_lstm_wide_library() if wide else capi.load_library()), actor_critic, torch.device(device)
        self._pre = "lg_lstm_wide_actor" if wide else "lg_lstm_actor"
        self._last_error = self.lib.lg_lstm_wide_last_error if wide else self.lib.lg_last_error
        self.seed, self.step_counter, self._host_step, self._out = int(seed), step_counter, 0, None
        lin = self._layers()
        dims = (C.c_int32 * 5)(lin[0].in_features, *[m.out_features for m in lin])
        self.num_actions = lin[3].out_features
        self.handle = C.c_void_p()
        rc = getattr(self.lib, self._pre + "_create")(dims, self.device.index or 0, C.byref(self.handle))
        if rc != 0:
            raise RuntimeError(f"{self._pre}_create failed ({rc}): {self._last_error().decode()}")
        self.sync_device()

    def _layers(self):
        mods = list(self.ac.actor)
        lin = [m for m in mods if isinstance(m, nn.Linear)]
        if len(lin) != 4 or not all(isinstance(m, nn.ELU) for m in mods if not isinstance(m, nn.Linear)):
            raise ValueError("the device actor supports 3 hidden layers with ELU (the reference's policy configs)")
        return lin

    def sync_device(self):
        lin = self._layers()
        for m in lin:
            if not (m.weight.is_cuda and m.weight.dtype == torch.float32 and m.weight.is_contiguous()):
                raise ValueError("DeviceLstmActor needs contiguous float32 CUDA parameters")
        ptr = C.c_void_p * 4
        rc = getattr(self.lib, self._pre + "_load_device")(self.handle, ptr(*[m.weight.data_ptr() for m in lin]), ptr(*[m.bias.data_ptr() for m in lin]),
                                                           self.ac.std.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream)
        if rc != 0:
            raise RuntimeError(f"{self._pre}_load_device failed ({rc}): {self._last_error().decode()}")

    # what HighLevelGame._act reads of a FusedActor (the shared actor launch writes into these buffers and counts its own launch)
    def output_buffers(self, n):
        """(actions, mean) tensors the kernels write into (re-used between calls; clone to keep a value)."""
        if self._out is None or self._out[0].shape[0] != n:
            self._out = (torch.empty(n, self.num_actions, device=self.device), torch.empty(n, self.num_actions, device=self.device))
        return self._out

    def peek_step(self):
        """``(step, step_counter)`` the next launch will use, without counting it (``FusedActor.peek_step``)."""
        if self.step_counter is not None:
            return -1, self.step_counter.data_ptr()
        return self._host_step + 1, None

    def next_step(self):
        """``peek_step`` and count the launch."""
        step, ctr = self.peek_step()
        if ctr is None:
            self._host_step = step
        return step, ctr

    def act_with_mean(self, h, deterministic=False):
        n = h.shape[0]
        actions, mean = self.output_buffers(n)
        step, ctr = self.next_step()
        rc = getattr(self.lib, self._pre + "_act")(self.handle, h.data_ptr(), actions.data_ptr(), mean.data_ptr(), n, self.seed, step, ctr,
                                                   int(deterministic), torch.cuda.current_stream(self.device).cuda_stream)
        if rc != 0:
            raise RuntimeError(f"{self._pre}_act failed ({rc}): {self._last_error().decode()}")
        return actions, mean

    def __del__(self):
        try:
            if self.handle:
                getattr(self.lib, self._pre + "_destroy")(self.handle)
                self.handle = C.c_void_p()
        except Exception:
            pass


class RecurrentFusedActor:
    """``FusedActor`` for an ``ActorCriticRecurrent``: owns the two ``lg_lstm`` handles, the ``(h, c)`` ping-pong buffers of both memories
    and the device actor MLP over ``actor_critic.actor`` (whose input width is ``rnn_hidden_size``).

    ``wide`` (the runner key ``wide_memory``): when either memory has more than 256 units, both memories and the actor take the handles of
    liblegged_lstm_wide.so (up to 512 units; one launch still advances both memories) and the attribute ``wide`` is True.  The game envs
    then issue the separate launches, because their shared kernels read main-library handles.  With both memories within 256 units
    nothing wide is created.

    ``gru`` (the runner key ``device_gru``): both memories are ``nn.GRU``; the cell handles are ``DeviceGru`` of liblegged_gru.so, the actor is
    the main library's and the attribute ``gru`` is True.  A GRU has one state tensor per memory: the slots hold 1-tuples ``(h,)`` where an
    LSTM's hold ``(h, c)``, and every method does for the one tensor what it does for the two.  ``dec_high_level_game`` then issues the
    separate launches, because its cell launch reads ``lg_lstm`` handles.  Without ``gru`` a GRU memory is refused as before.

    ``shared_gru`` (the runner key ``dec_gru_shared``, on top of ``gru``): the attribute ``shared_gru`` is True only when ``gru`` is; two such
    actors take ``lg_dec_gru_step`` (liblegged_dec_game_gru.so) -> ``lg_dec_game_lstm_act`` on ``dec_high_level_game``.  Nothing else reads it."""

    def __init__(self, actor_critic, device, seed: int = 1, step_counter: torch.Tensor = None, num_envs: int = None, wide: bool = False,
                 gru: bool = False, shared_gru: bool = False):
        if not getattr(actor_critic, "is_recurrent", False):
            raise ValueError("RecurrentFusedActor wraps an ActorCriticRecurrent")
        self.ac, self.device = actor_critic, torch.device(device)
        rnns = (actor_critic.memory_a.rnn, actor_critic.memory_c.rnn)
        self.gru = bool(gru) and all(isinstance(r, nn.GRU) for r in rnns)
        self.shared_gru = self.gru and bool(shared_gru)
        self.wide = not self.gru and bool(wide) and any(getattr(r, "hidden_size", 0) > capi.LG_LSTM_MAX_HIDDEN for r in rnns)
        if self.gru:
            self.lstm_a, self.lstm_c = DeviceGru(rnns[0], device), DeviceGru(rnns[1], device)
        else:
            self.lstm_a = DeviceLstm(rnns[0], device, wide=self.wide)
            self.lstm_c = DeviceLstm(rnns[1], device, wide=self.wide)
        self.fused = DeviceLstmActor(actor_critic, device, seed=seed, step_counter=step_counter, wide=self.wide)
        self.lib = capi.load_library()                          # the FusedActor surface: the main library (the runner's rollout bookkeeping)
        self.cell_lib = self.lstm_a.lib                         # the library of the cell handles: the main one, liblegged_lstm_wide.so or liblegged_gru.so
        self.num_envs, self._flip = None, 0
        if num_envs is not None:
            self._allocate(num_envs)

    # the FusedActor surface the runner reads
    seed = property(lambda self: self.fused.seed)
    step_counter = property(lambda self: self.fused.step_counter)
    num_actions = property(lambda self: self.fused.num_actions)
    # ... and what HighLevelGame._act reads: the actor MLP's handle, buffers and step count; the marker selects lg_game_lstm_act there
    recurrent = True
    gru = False                                                 # (the instance's, set by __init__: liblegged_gru.so handles, one state tensor per memory)
    shared_gru = False                                          # (likewise: the GRU pair of dec_high_level_game on the shared launches)
    handle = property(lambda self: self.fused.handle)

    def output_buffers(self, n):
        return self.fused.output_buffers(n)

    def peek_step(self):
        return self.fused.peek_step()

    def next_step(self):
        return self.fused.next_step()

    def _allocate(self, n):
        z = lambda h: torch.zeros(n, h, device=self.device)
        Ha, Hc = self.lstm_a.hidden, self.lstm_c.hidden
        st = (lambda h: (z(h),)) if self.gru else (lambda h: (z(h), z(h)))
        self.state_a = [st(Ha), st(Ha)]                        # [flip] -> (h, c), a GRU's (h,): the launch reads [flip] and writes [1 - flip]
        self.state_c = [st(Hc), st(Hc)]
        self.scratch_c = st(Hc)                                # outputs of a critic-only step that must not move the carried state
        self.num_envs, self._flip = n, 0
        self._critic_slots_equal = True                        # both slots of the critic memory hold the carried state (see advance_slots)

    def reset_states(self):
        for pair in self.state_a + self.state_c:
            for t in pair:
                t.zero_()
        self._critic_slots_equal = True

    def reset_critic_state(self):
        """Zero the critic memory's state in both slots (``DecGamePolicyRunner``: the agent that becomes the learner; the memory did not move
        while it was the opponent).  The actor memory carries on."""
        for pair in self.state_c:
            for t in pair:
                t.zero_()
        self._critic_slots_equal = True

    def hidden_states(self):
        """((h_a, c_a), (h_c, c_c)), a GRU's ((h_a,), (h_c,)), the next step starts from, as ``[1, N, H]`` views
        (``ActorCriticRecurrent.get_hidden_states``)."""
        return tuple(tuple(t.unsqueeze(0) for t in st[self._flip]) for st in (self.state_a, self.state_c))

    def publish_states(self, reset=None):
        """Point the torch module's memories at copies of the device state: the torch-side update and a later play start from the truth.
        ``reset``: the flags the next step would be given; the torch memories zero such rows at once (``Memory.reset``)."""
        st_a, st_c = self.hidden_states()
        keep = 1.0 if reset is None else (reset == 0).view(1, -1, 1).float()
        if self.gru:                                         # nn.GRU's state is the tensor, not a tuple
            self.ac.memory_a.hidden_states, self.ac.memory_c.hidden_states = st_a[0] * keep, st_c[0] * keep
            return
        self.ac.memory_a.hidden_states = tuple(t * keep for t in st_a)
        self.ac.memory_c.hidden_states = tuple(t * keep for t in st_c)

    def _cell_step(self, cell_a, cell_c, x_a, x_c, reset, in_a, out_a, in_c, out_c, n):
        """``lstm_step`` on ``(h, c)`` pairs or ``gru_step`` on the 1-tuples' tensors, on the current stream."""
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if self.gru:
            only = lambda st: None if st is None else st[0]
            gru_step(self.cell_lib, cell_a, cell_c, x_a, x_c, reset, only(in_a), only(out_a), only(in_c), only(out_c), n, stream)
        else:
            lstm_step(self.cell_lib, cell_a, cell_c, x_a, x_c, reset, in_a, out_a, in_c, out_c, n, stream)

    def step_memories(self, obs, critic_obs=None, reset=None):
        """Advance the actor memory (and, with ``critic_obs``, the critic memory) by one step; returns ``(h_a, h_c or None)``, the new
        outputs (buffers re-used two steps later).  ``reset``: bool / uint8 [N], rows that start from a zero state."""
        n = obs.shape[0]
        if self.num_envs != n:
            self._allocate(n)
        f = self._flip
        with_c = critic_obs is not None
        self._cell_step(self.lstm_a, self.lstm_c if with_c else None, self._f32(obs), self._f32(critic_obs) if with_c else None, self._flags(reset),
                        self.state_a[f], self.state_a[1 - f], self.state_c[f], self.state_c[1 - f], n)
        if not with_c:                                       # the critic memory did not move: keep both of its slots current
            for dst, src in zip(self.state_c[1 - f], self.state_c[f]):
                dst.copy_(src)
        self._critic_slots_equal = not with_c
        self._flip = 1 - f
        return self.state_a[1 - f][0], (self.state_c[1 - f][0] if with_c else None)

    def step_critic_memory(self, critic_obs, reset=None):
        """Advance the critic memory alone on this actor's slots (read ``[flip]``, write ``[1 - flip]``) and return its new output; the caller
        then calls ``advance_slots(True)`` (the separate launches of a pooled role, whose actor memory ``rl.RecurrentOpponentPool`` advances)."""
        f = self._flip
        self._cell_step(None, self.lstm_c, None, self._f32(critic_obs), self._flags(reset), None, None, self.state_c[f], self.state_c[1 - f],
                        critic_obs.shape[0])
        return self.state_c[1 - f][0]

    def cell_roles(self, n, x, critic_x=None, agent=""):
        """This actor's two role entries of a shared cell launch (``lg_dec_lstm_step`` / ``lg_dec_pool_lstm_step``, a GRU's ``lg_dec_gru_step``) on
        its own slots for ``n`` envs (allocated first when ``num_envs`` differs): the actor memory on ``x``, the critic memory on ``critic_x``
        or None.  An entry reads ``[flip]`` and writes ``[1 - flip]``: ``(handle, x, h_in, c_in, h_out, c_out)``, a GRU's
        ``(handle, x, h_in, h_out)``.  Returns ``(entries, h, critic output or None)``, the tensors the outputs land in; the caller issues the
        launch and then calls ``advance_slots`` (a warm-up call does not: the next step overwrites what it wrote)."""
        if self.num_envs != n:
            self._allocate(n)
        f, entries = self._flip, []
        for cell, state, inp in ((self.lstm_a, self.state_a, x), (self.lstm_c, self.state_c, critic_x)):
            if inp is not None and inp.shape[-1] != cell.num_in:
                raise ValueError(f"the {agent} agent's memory reads {cell.num_in} inputs, its input here has {inp.shape[-1]} (a critic memory reads "
                                 "the privileged observations where they are on)")
            entries.append(None if inp is None else (cell.handle, inp.data_ptr(), *(t.data_ptr() for t in state[f]), *(t.data_ptr() for t in state[1 - f])))
        return entries, self.state_a[1 - f][0], (None if critic_x is None else self.state_c[1 - f][0])

    def advance_slots(self, with_critic):
        """What ``step_memories`` does after its launch, for a caller that issued the launch itself on this actor's slots (``cell_roles``:
        read ``[flip]``, write ``[1 - flip]``).  A critic memory that did not move needs both of its slots
        current; they are copied only when the last step that moved it left them different, so a memory that never moves costs no copy."""
        f = self._flip
        if with_critic:
            self._critic_slots_equal = False
        elif not self._critic_slots_equal:
            for dst, src in zip(self.state_c[1 - f], self.state_c[f]):
                dst.copy_(src)
            self._critic_slots_equal = True
        self._flip = 1 - f

    def hold_slot(self):
        """Bring the state the last ``step_memories`` wrote back into the slots it read, and read from there again: a captured graph with an
        odd number of steps then starts every replay from the same addresses.  The returned outputs of that step stay valid."""
        f = self._flip
        for st in (self.state_a, self.state_c):
            for dst, src in zip(st[1 - f], st[f]):
                dst.copy_(src)
        self._critic_slots_equal = True
        self._flip = 1 - f

    def peek_critic(self, critic_obs, reset=None):
        """The critic memory's output for ``critic_obs`` from the carried state, which stays where it is (the last value of a rollout)."""
        n = critic_obs.shape[0]
        self._cell_step(None, self.lstm_c, None, self._f32(critic_obs), self._flags(reset), None, None, self.state_c[self._flip], self.scratch_c, n)
        return self.scratch_c[0]

    @staticmethod
    def _f32(t):
        return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()

    @staticmethod
    def _flags(reset):
        if reset is None:
            return None
        if reset.element_size() != 1:
            reset = (reset != 0).to(torch.uint8)
        return reset.contiguous()

    def act_with_mean(self, obs, critic_obs=None, reset=None, deterministic=False):
        """``(actions, mean)`` of one policy step; returns the critic memory's output as a third value when ``critic_obs`` is given."""
        h_a, h_c = self.step_memories(obs, critic_obs, reset)
        actions, mean = self.fused.act_with_mean(h_a, deterministic)
        return (actions, mean) if critic_obs is None else (actions, mean, h_c)

    def act(self, obs, reset=None):
        return self.act_with_mean(obs, reset=reset)[0]

    def act_inference(self, obs, reset=None):
        return self.act_with_mean(obs, reset=reset, deterministic=True)[0]

    def sync_device(self):
        """Refresh both memories and the actor from the torch parameters on the device; call after every optimiser step."""
        self.lstm_a.load_device()
        self.lstm_c.load_device()
        self.fused.sync_device()
