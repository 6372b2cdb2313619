"""PPO with GAE, clipped surrogate / value losses and the adaptive-KL learning rate
(hyper-parameters: reference ``legged_robot_config.py:215-228``)."""
import os

import torch
import torch.distributed as dist
import torch.nn as nn
import torch.optim as optim


def _world():
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def _switch(name):
    """An ``LG_*`` environment switch: on unless set to "0".  Read by the constructors only: a switch holds for the instance's life."""
    return os.environ.get(name, "1") != "0"


def gaussian_kl(mu, sig, old_mu, old_sig):
    """KL(old || new) of diagonal Gaussians per row (rsl_rl's expression)."""
    return torch.sum(torch.log(sig / old_sig + 1.0e-5) + (old_sig.square() + (old_mu - mu).square()) / (2.0 * sig.square()) - 0.5, dim=-1)


class RolloutStorage:
    class Transition:
        def __init__(self):
            self.clear()

        def clear(self):
            self.observations = self.critic_observations = self.actions = self.rewards = self.dones = None
            self.values = self.actions_log_prob = self.action_mean = self.action_sigma = None

    def __init__(self, num_envs, num_transitions_per_env, obs_shape, privileged_obs_shape, actions_shape, device="cpu"):
        T, N, self.device = num_transitions_per_env, num_envs, device
        z = lambda *s: torch.zeros(T, N, *s, device=device)
        self.observations = z(*obs_shape)
        self.privileged_observations = z(*privileged_obs_shape) if privileged_obs_shape[0] is not None else None
        self.rewards, self.dones = z(1), z(1).byte()
        self.actions, self.mu, self.sigma = z(*actions_shape), z(*actions_shape), z(*actions_shape)
        self.actions_log_prob, self.values, self.returns, self.advantages = z(1), z(1), z(1), z(1)
        self.num_transitions_per_env, self.num_envs, self.step = T, N, 0
        self.initial_hidden_a = self.initial_hidden_c = None      # recurrent policy: the state carried INTO the rollout, tuples of [layers, N, H]
        self._lib = None                                          # the HIP extension, loaded by the first GAE scan on a GPU

    def add_transitions(self, t):
        if self.step >= self.num_transitions_per_env:
            raise AssertionError("Rollout buffer overflow")
        i = self.step
        self.observations[i].copy_(t.observations)
        if self.privileged_observations is not None:
            self.privileged_observations[i].copy_(t.critic_observations)
        self.actions[i].copy_(t.actions)
        self.rewards[i].copy_(t.rewards.view(-1, 1))
        self.dones[i].copy_(t.dones.view(-1, 1))
        self.values[i].copy_(t.values)
        self.actions_log_prob[i].copy_(t.actions_log_prob.view(-1, 1))
        self.mu[i].copy_(t.action_mean)
        self.sigma[i].copy_(t.action_sigma)
        self.step += 1

    def clear(self):
        self.step = 0

    def save_initial_hidden_states(self, hidden_states):
        """Recurrent policy: the (actor, critic) memory states at the first step of the rollout, ``None`` for a memory that has not stepped
        yet (zeros).  Stored once per rollout: every later trajectory of an env starts behind a done, i.e. from zeros, so rsl_rl's
        per-step copies (4 x T x N x H floats) carry nothing these 4 x N x H do not."""
        def stored(old, hid):
            if hid is None:
                for o in old or ():
                    o.zero_()
                return old
            hid = hid if isinstance(hid, tuple) else (hid,)
            if old is None or len(old) != len(hid) or any(o.shape != h.shape for o, h in zip(old, hid)):
                old = tuple(torch.zeros(h.shape, device=self.device) for h in hid)       # (fixed buffers: a captured rollout copies into them)
            for o, h in zip(old, hid):
                o.copy_(h)
            return old
        hid_a, hid_c = hidden_states
        self.initial_hidden_a, self.initial_hidden_c = stored(self.initial_hidden_a, hid_a), stored(self.initial_hidden_c, hid_c)

    def recurrent_mini_batch_generator(self, num_mini_batches, num_epochs=8):
        """rsl_rl's generator of the same name: mini-batches are contiguous env ranges; every env's rollout is cut behind each done into
        trajectories, ordered env-major, padded to T and masked.  ``obs`` / ``cobs`` are [T, n_traj, .], everything else [T, mb_envs, .];
        the hidden states are the initial state per trajectory [layers, n_traj, H]: the stored carried-in state for an env's first
        trajectory, zeros for the others."""
        from .actor_critic import split_and_pad_trajectories
        T, N = self.num_transitions_per_env, self.num_envs
        obs_all, masks_all = split_and_pad_trajectories(self.observations, self.dones)
        cobs_all = split_and_pad_trajectories(self.privileged_observations, self.dones)[0] if self.privileged_observations is not None else obs_all
        dones = self.dones.view(T, N) != 0
        starts = torch.zeros_like(dones)
        starts[1:] = dones[:-1]
        starts[0] = True
        per_env = starts.sum(0)                                        # trajectories per env
        first = torch.cumsum(per_env, 0) - per_env                     # index of each env's first trajectory
        n_traj = int(per_env.sum())

        def initial(stored):
            if stored is None:
                return None
            out = tuple(s.new_zeros(s.shape[0], n_traj, s.shape[2]) for s in stored)
            for o, s in zip(out, stored):
                o[:, first] = s
            return out
        hid_a_all, hid_c_all = initial(self.initial_hidden_a), initial(self.initial_hidden_c)
        pick = lambda hid, a, b: None if hid is None else (tuple(h[:, a:b].contiguous() for h in hid) if len(hid) > 1 else hid[0][:, a:b].contiguous())
        mb = N // num_mini_batches                                     # (the tail envs of an uneven split are dropped, as rsl_rl does)
        for _ in range(num_epochs):
            for i in range(num_mini_batches):
                a, b = i * mb, (i + 1) * mb
                ta, tb = int(first[a]), int(first[b - 1] + per_env[b - 1])
                yield (obs_all[:, ta:tb], cobs_all[:, ta:tb], self.actions[:, a:b], self.values[:, a:b], self.advantages[:, a:b], self.returns[:, a:b],
                       self.actions_log_prob[:, a:b], self.mu[:, a:b], self.sigma[:, a:b], (pick(hid_a_all, ta, tb), pick(hid_c_all, ta, tb)), masks_all[:, ta:tb])

    def compute_returns(self, last_values, gamma, lam):
        """GAE(gamma, lambda); advantages normalised over the GLOBAL batch: with several ranks
        the fused [returns || advantages] buffer is all-gathered once (RCCL over xGMI)."""
        if not self._gae_kernel(last_values, gamma, lam):
            self._gae_torch(last_values, gamma, lam)
        self._normalise_advantages()

    def _gae_kernel(self, last_values, gamma, lam):
        """One launch of the HIP scan (``lg_gae_returns``) instead of ~6 torch kernels per rollout step; GPU only."""
        if not self.values.is_cuda:
            return False
        if self._lib is None:
            from .. import capi
            self._lib = capi.load_library()        # on a GPU the extension is the product path: a missing build fails loudly here
        T, N = self.num_transitions_per_env, self.num_envs
        lv = last_values.reshape(-1).contiguous().float()
        rc = self._lib.lg_gae_returns(self.rewards.data_ptr(), self.values.data_ptr(), self.dones.data_ptr(), lv.data_ptr(), float(gamma), float(lam),
                                      self.returns.data_ptr(), self.advantages.data_ptr(), T, N, torch.cuda.current_stream(self.values.device).cuda_stream)
        if rc != 0:
            raise RuntimeError(f"lg_gae_returns failed ({rc}): {self._lib.lg_last_error().decode()}")
        return True

    def _gae_torch(self, last_values, gamma, lam):
        adv = 0
        for step in reversed(range(self.num_transitions_per_env)):
            nxt = last_values if step == self.num_transitions_per_env - 1 else self.values[step + 1]
            # (tests/test_ppo_tail_ref.py drives this scan on double tensors and stands in for `dones`: it answers `[step].float()` only --
            # read the flags another way and that test fails with an AttributeError until its stand-in follows)
            not_done = 1.0 - self.dones[step].float()
            delta = self.rewards[step] + not_done * gamma * nxt - self.values[step]
            adv = delta + not_done * gamma * lam * adv
            self.returns[step] = adv + self.values[step]
        torch.sub(self.returns, self.values, out=self.advantages)        # in place: a captured update graph reads this buffer

    def _normalise_advantages(self):
        if _world() > 1:
            fused = torch.cat((self.returns.flatten(), self.advantages.flatten()))
            gathered = torch.empty(_world() * fused.numel(), device=fused.device, dtype=fused.dtype)
            dist.all_gather_into_tensor(gathered, fused)
            all_adv = gathered.view(_world(), 2, -1)[:, 1, :]
            mean, std = all_adv.mean(), all_adv.std()
        else:
            mean, std = self.advantages.mean(), self.advantages.std()
        self.advantages.sub_(mean).div_(std + 1e-8)

    def get_statistics(self):
        done = self.dones.clone()
        done[-1] = 1
        flat = done.permute(1, 0, 2).reshape(-1, 1)
        idx = torch.cat((flat.new_tensor([-1], dtype=torch.int64), flat.nonzero(as_tuple=False)[:, 0]))
        lens = idx[1:] - idx[:-1]
        return lens.float().mean(), self.rewards.mean()

    def flat_views(self):
        """The stored rollout as [T * N, .] views, in the order the mini-batch tuples use: obs, critic obs (the SAME view as obs when no
        privileged observations are stored), actions, values, advantages, returns, log-probabilities, mu, sigma."""
        obs = self.observations.flatten(0, 1)
        cobs = self.privileged_observations.flatten(0, 1) if self.privileged_observations is not None else obs
        return (obs, cobs, self.actions.flatten(0, 1), self.values.flatten(0, 1), self.advantages.flatten(0, 1), self.returns.flatten(0, 1),
                self.actions_log_prob.flatten(0, 1), self.mu.flatten(0, 1), self.sigma.flatten(0, 1))

    def mini_batch_generator(self, num_mini_batches, num_epochs=8, perm=None):
        B = self.num_envs * self.num_transitions_per_env
        mb = B // num_mini_batches
        if perm is None:
            perm = torch.randperm(num_mini_batches * mb, requires_grad=False, device=self.device)
        flat = self.flat_views()
        for _ in range(num_epochs):
            for i in range(num_mini_batches):
                ix = perm[i * mb:(i + 1) * mb]
                yield (*(t[ix] for t in flat), (None, None), None)


class _LinearSplitK(torch.autograd.Function):
    """``F.linear`` whose weight gradient is computed as a batched GEMM over row chunks.  dW = g^T x has the whole mini-batch
    (24 576 rows) as its K dimension and only out x in <= 512 x 512 outputs: hipBLASLt runs it on 16 workgroups (324 us for
    512 x 235); cutting the rows into S chunks gives S times the tiles (torch.bmm) and a cheap [S, out, in] sum."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return torch.addmm(b, x, w.t())

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        M = x.shape[0]
        S = next((s for s in (16, 12, 8, 6, 4, 3, 2) if M % s == 0 and M // s >= 256), 1)
        g = g.contiguous()
        if S > 1:
            gw = torch.bmm(g.view(S, M // S, -1).transpose(1, 2), x.view(S, M // S, -1)).sum(0)
        else:
            gw = g.t() @ x
        gx = g @ w if ctx.needs_input_grad[0] else None
        return gx, gw, g.sum(0)


def _mlp_split_k(seq, x):
    """Apply an ``nn.Sequential`` of Linear / activation modules with ``_LinearSplitK`` in place of ``nn.Linear``."""
    for m in seq:
        x = _LinearSplitK.apply(x, m.weight, m.bias) if isinstance(m, nn.Linear) else m(x)
    return x


class PPO:
    """The ``LG_PPO_*`` switches and ``LG_DP_GRAPHS`` are read once, by the constructor: they hold per instance, so set them before
    constructing ``PPO`` (``LG_DP_GRAPHS=0``: the data-parallel kernel update keeps its eager launches -- A/B, and what a refused capture
    falls back to).  The structure of the device update is described in DESIGN.md ("The update's driver")."""

    def __init__(self, actor_critic, num_learning_epochs=1, num_mini_batches=1, clip_param=0.2, gamma=0.998, lam=0.95,
                 value_loss_coef=1.0, entropy_coef=0.0, learning_rate=1e-3, max_grad_norm=1.0,
                 use_clipped_value_loss=True, schedule="fixed", desired_kl=0.01, device="cpu", graphed_update=True, fused_loss=True, device_bptt=False):
        self.device = device
        # Single-GPU runs replay one captured HIP graph per mini-batch step (forward, losses, backward, grad clip, Adam and
        # the adaptive-KL learning rate all on the device): the flat networks' update is launch-bound (~150 tiny kernels).
        # (a recurrent policy is updated by the eager loop of update(): back-propagation through time is autograd's)
        self._graph_ok = bool(graphed_update) and str(device).startswith("cuda") and not getattr(actor_critic, "is_recurrent", False)
        # ... and the surrogate / value / entropy losses with their gradients w.r.t. the network outputs come from ONE HIP kernel
        # (``lg_ppo_loss``) instead of ~100 small torch kernels; autograd only runs through the two MLPs.
        self._fused_loss = bool(fused_loss) and self._graph_ok and _switch("LG_PPO_FUSED_LOSS")
        # ... and for the MLP shape of the flat tasks the two networks' forward and backward run in the MFMA learner kernels
        # (lg_mlp_forward / lg_mlp_backward, rl/mlp_kernels.py): autograd is not involved at all.  LG_PPO_MLP_KERNELS=0 disables.
        self._mlp_kernels = self._fused_loss and _switch("LG_PPO_MLP_KERNELS")
        # ... and gradient clipping, the adaptive-KL learning-rate rule and Adam are two launches (lg_adam_step) instead of ~60
        # small torch kernels, updating torch.optim.Adam's own state tensors in place.  LG_PPO_ADAM_KERNEL=0 disables.
        self._adam_kernel = self._fused_loss and _switch("LG_PPO_ADAM_KERNEL")
        self._fused_minibatch = _switch("LG_PPO_FUSED_MINIBATCH")     # lg_ppo_minibatch instead of forward / loss / backward
        self._wide_kernels = _switch("LG_PPO_WIDE_KERNELS")           # lg_mlp_wide_* for widths the LDS-resident kernels do not cover
        self._split_k = _switch("LG_PPO_SPLIT_K")                     # torch MLP path (wide networks): see _LinearSplitK
        self._dp_graphs_wanted = _switch("LG_DP_GRAPHS")              # world_size > 1: capture the two halves around the all-reduce
        # What is captured over fixed addresses (_drop_captured lets go of all of it, and nothing else does):
        self._graph, self._graph_whole = None, False     # one process: the update graph; whole = epochs x mini-batches in ONE graph
        self._dp_graphs = None                           # several: ([pre graph per mini-batch slot], post graph); False = capture refused
        self._mlp, self._mlp_key = None, None            # MlpTrainer (descriptors hold parameter / .grad / storage addresses)
        self._dp_key = None                        # _capture_key() of the last update
        self._updates_done = 0                           # 0: the next update is the eager warm-up, >= 1: capture may happen
        self._dp_graph_error = "not attempted (LG_DP_GRAPHS=0 or the torch MLP path)"      # why the two graphs are not in use; None: they are
        self.dp_launches = None
        # Device buffers of an update (_ensure_buffers) and the flat gradient buffer of the data-parallel kernel path (_flat_grad_views):
        self._buffers_key = None
        self._perm_buf = self._ix_one = self._acc = self._stats = self._d_std = self._d_mu = self._d_val = None
        self._adam_scratch = self._gstream = None
        self._gflat, self._goffs = None, None
        self._lib = None
        self.desired_kl, self.schedule, self.learning_rate = desired_kl, schedule, learning_rate
        self.actor_critic = actor_critic.to(device)
        if device_bptt:
            self._attach_device_bptt()
        self.storage = None
        self._prime = self._lr = None
        if self._graph_ok:
            # The CUDA generator allocates its graph-safe state tensors at the first capture in the process; if that happens
            # under torch.inference_mode (the rollout graph, rl/runner.py) they become inference tensors and a later capture
            # with autograd enabled cannot touch them.  Prime them here, in normal mode.
            # (kept alive: the generator drops the tensors again when its last graph goes away)
            self._prime = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._prime, capture_error_mode="thread_local"):
                torch.zeros(1, device=device).add_(1.0)
            self._lr = torch.tensor(float(learning_rate), device=device)
            self.optimizer = optim.Adam(self.actor_critic.parameters(), lr=self._lr, capturable=True)
        else:
            self.optimizer = optim.Adam(self.actor_critic.parameters(), lr=learning_rate)
        self.transition = RolloutStorage.Transition()
        self.clip_param, self.num_learning_epochs, self.num_mini_batches = clip_param, num_learning_epochs, num_mini_batches
        self.value_loss_coef, self.entropy_coef = value_loss_coef, entropy_coef
        self.gamma, self.lam, self.max_grad_norm = gamma, lam, max_grad_norm
        self.use_clipped_value_loss = use_clipped_value_loss

    def _attach_device_bptt(self):
        """``device_bptt``: the recurrence of both memories' batch mode on the LSTM sequence kernels (rl/lstm_sequence.py) instead of
        ``nn.LSTM`` and autograd's back-propagation through time; the update loop itself is the same.  Both memories or neither."""
        ac = self.actor_critic
        if not getattr(ac, "is_recurrent", False):
            why = "the policy is not recurrent"
        elif not str(self.device).startswith("cuda"):
            why = f"the learner is on {self.device}"
        else:
            from .lstm_sequence import sequence_unsupported_reason
            why = sequence_unsupported_reason(ac.memory_a.rnn) or sequence_unsupported_reason(ac.memory_c.rnn)
        if why is not None:
            print(f"[ppo] device BPTT unavailable ({why}); torch LSTM and autograd in the update")
            return
        from .lstm_sequence import DeviceLstmSequence
        ac.memory_a.sequence = DeviceLstmSequence(ac.memory_a.rnn, self.device)
        ac.memory_c.sequence = DeviceLstmSequence(ac.memory_c.rnn, self.device)

    def init_storage(self, num_envs, num_transitions_per_env, actor_obs_shape, critic_obs_shape, action_shape):
        self.storage = RolloutStorage(num_envs, num_transitions_per_env, actor_obs_shape, critic_obs_shape, action_shape, self.device)

    def test_mode(self):
        self.actor_critic.eval()

    def train_mode(self):
        self.actor_critic.train()

    def act(self, obs, critic_obs):
        t = self.transition
        first = self.actor_critic.is_recurrent and self.storage.step == 0
        carried = self.actor_critic.get_hidden_states() if first else None
        t.actions = self.actor_critic.act(obs).detach()
        t.values = self.actor_critic.evaluate(critic_obs).detach()
        if first:                                    # the state this rollout starts from; memories that had not stepped yet started from zeros
            zeros = lambda hid: tuple(torch.zeros_like(h) for h in hid) if isinstance(hid, tuple) else torch.zeros_like(hid)
            self.storage.save_initial_hidden_states([zeros(now) if was is None else was for was, now in zip(carried, self.actor_critic.get_hidden_states())])
        t.actions_log_prob = self.actor_critic.get_actions_log_prob(t.actions).detach()
        t.action_mean = self.actor_critic.action_mean.detach()
        t.action_sigma = self.actor_critic.action_std.detach()
        t.observations, t.critic_observations = obs, critic_obs
        return t.actions

    def process_env_step(self, rewards, dones, infos):
        t = self.transition
        t.rewards = rewards.clone()
        t.dones = dones
        if "time_outs" in infos:      # bootstrap on time-outs (the env sends them: legged_robot.py:190-191)
            t.rewards += self.gamma * torch.squeeze(t.values * infos["time_outs"].unsqueeze(1).to(self.device), 1)
        self.storage.add_transitions(t)
        t.clear()
        self.actor_critic.reset(dones)

    def compute_returns(self, last_critic_obs, last_values=None):
        """``last_values``: the caller already has critic(last_critic_obs) (the runner's device rollout of a recurrent policy)."""
        if last_values is not None:
            return self.storage.compute_returns(last_values, self.gamma, self.lam)
        ac = self.actor_critic
        carried = ac.memory_c.hidden_states if ac.is_recurrent else None
        last_values = ac.evaluate(last_critic_obs).detach()
        if ac.is_recurrent:
            # the critic's memory stays where the rollout left it: the next rollout feeds it this observation again (rsl_rl lets
            # this call advance it, so its critic sees the observation twice)
            ac.memory_c.hidden_states = carried
        self.storage.compute_returns(last_values, self.gamma, self.lam)

    # ------------------------------------------------------------------ one body per formula
    @property
    def _adaptive(self):
        return self.desired_kl is not None and self.schedule == "adaptive"

    def _loss(self, lp, old_lp, adv, val, tval, ret, entropy):
        """(total loss, clipped surrogate, value loss) of a mini-batch; ``old_lp`` / ``adv`` arrive squeezed to the shape of ``lp``."""
        ratio = torch.exp(lp - old_lp)
        surrogate = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - self.clip_param, 1.0 + self.clip_param)).mean()
        if self.use_clipped_value_loss:
            vclip = tval + (val - tval).clamp(-self.clip_param, self.clip_param)
            vloss = torch.max((val - ret).pow(2), (vclip - ret).pow(2)).mean()
        else:
            vloss = (ret - val).pow(2).mean()
        return surrogate + self.value_loss_coef * vloss - self.entropy_coef * entropy.mean(), surrogate, vloss

    @torch.no_grad()
    def _kl_rule(self, kl):
        """The adaptive-KL rule on the DEVICE learning rate (no host decision: capturable).  The eager loop of update() applies the same
        rule to Python floats and ``param_groups``: another mechanism, kept there."""
        lr = self._lr
        down, up = torch.clamp(lr / 1.5, min=1e-5), torch.clamp(lr * 1.5, max=1e-2)
        self._lr.copy_(torch.where(kl > self.desired_kl * 2.0, down, torch.where((kl < self.desired_kl / 2.0) & (kl > 0.0), up, lr)))

    def _loss_inputs(self):
        """The seven storage tables and four coefficients of lg_ppo_loss and of struct lg_ppo_batch, in the order both take them."""
        st, p = self.storage, lambda t: t.data_ptr()
        return ((p(st.actions), p(st.actions_log_prob), p(st.mu), p(st.sigma), p(st.advantages), p(st.values), p(st.returns)),
                (float(self.clip_param), float(self.value_loss_coef), float(self.entropy_coef), int(bool(self.use_clipped_value_loss))))

    # ------------------------------------------------------------------ device state: buffers, flat gradients, what is captured
    def _ensure_buffers(self, mb, nmb, num_actions):
        """The device buffers an update works in, allocated together and again only when a size changes; True when that happened."""
        key = (mb, nmb, num_actions)
        if key == self._buffers_key:
            return False
        dev = self.device
        # mini-batch i reads rows _perm_buf[i*mb : (i+1)*mb]: fixed addresses, so captured kernels need no index copies
        self._perm_buf = torch.zeros(nmb * mb, dtype=torch.int64, device=dev)
        self._ix_one = torch.zeros(mb, dtype=torch.int64, device=dev)          # row list of the one-step graph
        self._acc = torch.zeros(2, device=dev)                                 # running sums of (value loss, surrogate) over the update
        self._stats = torch.zeros(4, device=dev)                               # a step's (surrogate, value loss, KL, entropy)
        # d loss / d (std, mu, value) from lg_ppo_loss.  _d_std is owned here; _flat_grad_views re-points it into the flat buffer.
        self._d_std = torch.zeros(num_actions, device=dev)
        self._d_mu, self._d_val = torch.empty(mb, num_actions, device=dev), torch.empty(mb, 1, device=dev)
        if self._adam_kernel and self._adam_scratch is None:
            from .. import capi
            self._adam_scratch = torch.zeros(capi.LG_ADAM_SCRATCH_FLOATS, device=dev)
        if self._gstream is None:
            self._gstream = torch.cuda.Stream(device=dev)                      # warm-up and capture run on it
        self._buffers_key = key
        return True

    def _flat_grad_views(self):
        """Data-parallel kernel path: every parameter's ``.grad`` (and the policy-std gradient the loss kernel writes) becomes a
        view of ONE persistent flat buffer, with one extra slot for the mean KL.  The learner kernels then write their gradients
        straight into that buffer and a mini-batch step needs a single all-reduce over it (RCCL: one collective of
        n_params + 1 floats instead of a concatenation, an all-reduce, a scalar all-reduce and 17 copies back)."""
        params = list(self.actor_critic.parameters())
        n = sum(p.numel() for p in params)
        buf = self._gflat
        if buf is None or buf.numel() != n + 1 or any(p.grad is None or p.grad.data_ptr() != buf[o].data_ptr() for p, o in zip(params, self._goffs)):
            buf = torch.zeros(n + 1, device=self.device)
            offs, o = [], 0
            for p in params:
                if p.grad is not None:
                    buf[o:o + p.numel()].copy_(p.grad.reshape(-1))
                p.grad = buf[o:o + p.numel()].view_as(p)
                offs.append(o)
                o += p.numel()
            self._gflat, self._goffs = buf, offs
            self._drop_captured(warm_up_again=False)     # descriptors and graphs hold the old .grad addresses
        # The one writer of _d_std besides _ensure_buffers: on this path the loss kernels write d loss / d std into the buffer's std slot
        # (on every call: _ensure_buffers hands out a fresh tensor when the storage changes size, the slot stays).
        self._d_std = self.actor_critic.std.grad
        return self._gflat

    def _dp_state_key(self):
        """Addresses a captured update bakes in besides the storage's: Adam's state tensors and the flat gradient buffer."""
        ptrs = []
        for q in self.actor_critic.parameters():
            stt = self.optimizer.state.get(q) or {}
            ptrs += [stt[k].data_ptr() if torch.is_tensor(stt.get(k)) else 0 for k in ("exp_avg", "exp_avg_sq", "step")]
        return tuple(ptrs) + (self._gflat.data_ptr() if self._gflat is not None else 0,)

    def _capture_key(self, mb):
        """The one key of everything captured: the storage's addresses, the mini-batch size and ``_dp_state_key``."""
        st = self.storage
        return (st.observations.data_ptr(), st.advantages.data_ptr(), st.returns.data_ptr(), mb) + self._dp_state_key()

    def _drop_captured(self, warm_up_again):
        """THE invalidation point: everything captured over addresses that are no longer the live ones goes -- both kinds of graphs, their
        key, the MlpTrainer's descriptors.  ``warm_up_again``: the next update runs eagerly first (it re-creates what a capture must not)."""
        self._graph, self._graph_whole, self._dp_graphs, self._dp_key, self._mlp = None, False, None, None, None
        if warm_up_again:
            self._updates_done = 0

    def after_optimizer_load(self):
        """The optimiser's tensors were replaced (checkpoint resume): re-link the device learning rate and drop what was captured
        (the Adam launches of the graphs hold the old state addresses)."""
        if self._graph_ok:
            for g in self.optimizer.param_groups:
                self._lr.copy_(torch.as_tensor(g["lr"], device=self.device).float().reshape(()))
                g["lr"] = self._lr
            self._drop_captured(warm_up_again=True)

    def _fused_ready(self):
        if not self._fused_loss:
            return False
        if self._lib is None:
            from .. import capi
            self._lib = capi.load_library()        # cuda device: no silent torch substitute for a missing extension
        ac = self.actor_critic
        return bool(self._lib) and hasattr(ac, "actor") and hasattr(ac, "critic") and hasattr(ac, "std") and ac.std.numel() <= 16

    def _mlp_trainer(self, mb):
        """MlpTrainer for the current storage / mini-batch size, or None when the networks are not the kernels' shape."""
        if not self._mlp_kernels:
            return None
        ac = self.actor_critic
        obs, cobs = self.storage.flat_views()[:2]
        key = (obs.data_ptr(), cobs.data_ptr(), mb)
        if self._mlp is None or self._mlp_key != key:
            from .mlp_kernels import MlpTrainer, WideMlpTrainer
            nets, tr = [ac.actor, ac.critic], None
            if all(isinstance(n, nn.Sequential) for n in nets):
                tr = MlpTrainer(nets, [obs, cobs], mb)
                if not tr.supported and self._wide_kernels:      # not the LDS-resident shape: the layer-wise GEMM kernels take any widths
                    tr = WideMlpTrainer(nets, [obs, cobs], mb)
            self._mlp, self._mlp_key = (tr if tr is not None and tr.supported else None), key
            self._mlp_kernels = self._mlp is not None            # no kernels for these networks: the torch MLP path from here on
        return self._mlp

    def _adam_table(self):
        """lg_adam_tensor[] over torch.optim.Adam's parameters and state, or None while the state does not exist yet (the very
        first step is torch's: it creates exp_avg / exp_avg_sq / step) or the optimiser is not plain capturable Adam."""
        from .. import capi
        opt = self.optimizer
        if len(opt.param_groups) != 1:
            return None
        g = opt.param_groups[0]
        if g.get("amsgrad") or g.get("weight_decay") or g.get("maximize") or not g.get("capturable") or g["lr"] is not self._lr:
            return None
        params = [q for q in g["params"] if q.grad is not None]
        if not params or len(params) > 32:
            return None
        table = (capi.lg_adam_tensor * len(params))()
        for i, q in enumerate(params):
            stt = opt.state.get(q)
            if not stt or "exp_avg" not in stt or not torch.is_tensor(stt["step"]) or stt["step"].dtype != torch.float32 \
                    or not stt["step"].is_cuda or q.dtype != torch.float32 or not q.is_contiguous() or not q.grad.is_contiguous():
                return None
            t = table[i]
            t.param, t.grad, t.exp_avg, t.exp_avg_sq = q.data_ptr(), q.grad.data_ptr(), stt["exp_avg"].data_ptr(), stt["exp_avg_sq"].data_ptr()
            t.step, t.numel = stt["step"].data_ptr(), q.numel()
        return table

    # ------------------------------------------------------------------ the mini-batch step, in three parts
    def _gradients(self, ix):
        """Part 1: MLP forward -> PPO loss -> MLP backward on the rows ``ix``.  ONE kernel (lg_ppo_minibatch) when the networks have the
        learner kernels' shape; otherwise wide learner kernels or torch MLP passes (autograd) around lg_ppo_loss.  Returns (flat, acc_done):
        the gradients lie in the data-parallel flat buffer (its last slot then carries the KL) / the kernel already summed the losses."""
        st, ac = self.storage, self.actor_critic
        if _world() > 1 and self._mlp_kernels:
            self._flat_grad_views()                  # .grad tensors = views of one buffer (before the descriptors read their addresses)
        tr = self._mlp_trainer(ix.numel())
        flat = _world() > 1 and tr is not None       # (torch MLP path: autograd allocates its own .grad tensors)
        p = lambda t: t.data_ptr()
        tables, coefs = self._loss_inputs()
        acc_done = tr is not None and self._fused_minibatch and tr.has_fused_minibatch
        if acc_done:
            # forward + loss + backward of both networks in ONE kernel: mu / value never reach HBM, and it keeps the running loss sums
            tr.refresh()
            from .. import capi
            tr.ppo_minibatch(ix, capi.lg_ppo_batch(*tables, p(ac.std), *coefs, p(self._d_std), p(self._stats), p(self._acc)))
        else:
            if tr is not None:
                tr.refresh()                         # parameter / .grad addresses (stable in steady state)
                mu, val = tr.forward(ix)
                d_mu, d_val = tr.grad_outputs
            else:
                obs_all, cobs_all = st.flat_views()[:2]
                obs = obs_all[ix]
                cobs = obs if cobs_all is obs_all else cobs_all[ix]
                if self._split_k and isinstance(ac.actor, nn.Sequential) and isinstance(ac.critic, nn.Sequential):
                    mu, val = _mlp_split_k(ac.actor, obs), _mlp_split_k(ac.critic, cobs)
                else:
                    mu, val = ac.actor(obs), ac.critic(cobs)
                d_mu, d_val = self._d_mu, self._d_val
            mb, A = mu.shape
            rc = self._lib.lg_ppo_loss(p(mu), p(ac.std), p(val), p(ix), *tables, *coefs, p(d_mu), p(self._d_std), p(d_val), p(self._stats),
                                       int(mb), int(A), torch.cuda.current_stream(mu.device).cuda_stream)
            if rc != 0:
                raise RuntimeError(f"lg_ppo_loss failed ({rc}): {self._lib.lg_last_error().decode()}")
            if tr is not None:
                tr.backward(ix)
            else:
                torch.autograd.backward([mu, val], [d_mu, d_val])
        ac.std.grad = self._d_std
        if flat and self._adaptive:
            self._gflat[-1:].copy_(self._stats[2:3])
        return flat, acc_done

    def _collective(self, flat):
        """Part 2: sum over the ranks -- ONE all-reduce of the flat buffer (gradients + KL slot; ``_optimise`` takes the mean), or the
        concatenate / all-reduce / copy-back of autograd's ``.grad`` tensors and a scalar all-reduce of the KL."""
        if flat:
            dist.all_reduce(self._gflat, op=dist.ReduceOp.SUM)
        elif _world() > 1:
            self._allreduce_grads()
            if self._adaptive:
                dist.all_reduce(self._stats[2:3], op=dist.ReduceOp.SUM)
                self._stats[2:3] /= _world()

    def _allreduce_grads(self):
        if _world() == 1:
            return
        grads = [p.grad for p in self.actor_critic.parameters() if p.grad is not None]
        flat = torch.cat([g.flatten() for g in grads])
        dist.all_reduce(flat, op=dist.ReduceOp.SUM)
        flat /= _world()
        o = 0
        for g in grads:
            g.copy_(flat[o:o + g.numel()].view_as(g))
            o += g.numel()

    def _optimise(self, flat, acc_done):
        """Part 3: [mean over the ranks of the all-reduced flat buffer] -> gradient clip + KL rule + Adam -> running loss sums."""
        adaptive, p = self._adaptive, lambda t: t.data_ptr()
        if flat:
            self._gflat.mul_(1.0 / _world())
            if adaptive:
                self._stats[2:3].copy_(self._gflat[-1:])
        table = self._adam_table() if self._adam_kernel else None
        if table is not None:
            g = self.optimizer.param_groups[0]
            rc = self._lib.lg_adam_step(table, len(table), p(self._lr), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                                        float(self.max_grad_norm), p(self._stats[2:]) if adaptive else None,
                                        float(self.desired_kl) if adaptive else 0.0, p(self._adam_scratch),
                                        torch.cuda.current_stream(self.device).cuda_stream)
            if rc != 0:
                raise RuntimeError(f"lg_adam_step failed ({rc}): {self._lib.lg_last_error().decode()}")
        else:
            if adaptive:
                self._kl_rule(self._stats[2])
            nn.utils.clip_grad_norm_(self.actor_critic.parameters(), self.max_grad_norm)
            self.optimizer.step()
        if not acc_done:
            with torch.no_grad():
                self._acc[0] += self._stats[1]
                self._acc[1] += self._stats[0]

    def _mb_step_torch(self, ix):
        """The step without the loss kernel (``fused_loss=False``; one process): torch's loss and autograd, still without host decisions."""
        obs, cobs, act, tval, adv, ret, old_lp, old_mu, old_sig = (t[ix] for t in self.storage.flat_views())
        ac = self.actor_critic
        ac.update_distribution(obs)
        lp = ac.get_actions_log_prob(act)
        val = ac.evaluate(cobs)
        mu, sig, ent = ac.action_mean, ac.action_std, ac.entropy
        if self._adaptive:
            with torch.no_grad():
                self._kl_rule(gaussian_kl(mu, sig, old_mu, old_sig).mean())
        loss, surrogate, vloss = self._loss(lp, torch.squeeze(old_lp), torch.squeeze(adv), val, tval, ret, ent)
        loss.backward()
        nn.utils.clip_grad_norm_(self.actor_critic.parameters(), self.max_grad_norm)
        self.optimizer.step()
        with torch.no_grad():
            self._acc[0] += vloss.detach()
            self._acc[1] += surrogate.detach()

    def _mb_step(self, ix):
        """One mini-batch step on the rows ``ix``; everything stays on the device (no host decisions)."""
        if not self._fused_ready():
            return self._mb_step_torch(ix)
        flat, acc_done = self._gradients(ix)
        self._collective(flat)
        self._optimise(flat, acc_done)

    def _zero_grad(self):
        # the learner kernels overwrite persistent .grad tensors (their addresses are baked into the captured graph)
        if not (self._mlp_kernels and self._mlp is not None):
            self.optimizer.zero_grad(set_to_none=True)

    # ------------------------------------------------------------------ the schedule of a device update
    def _begin_update(self, perm):
        """Buffers, the check of what was captured, accumulator reset, permutation copy; returns each mini-batch's rows (views of ``_perm_buf``)."""
        st, nmb = self.storage, self.num_mini_batches
        mb = st.num_envs * st.num_transitions_per_env // nmb
        resized = self._ensure_buffers(mb, nmb, st.actions.shape[-1])
        key = self._capture_key(mb)
        if (resized or key != self._dp_key) and (self._graph is not None or self._dp_graphs is not None):
            # Captured over other addresses (the storage was re-allocated).  One process warms up eagerly again before re-capturing;
            # the data-parallel capture prepares its trainer outside the graphs and captures again in this update.
            # (a key that changes while nothing is captured -- Adam's state appears during update 0 -- restarts nothing)
            self._drop_captured(warm_up_again=_world() == 1)
        self._dp_key = key
        self._acc.zero_()
        if perm is None:                             # one permutation per update, re-used by every epoch (rsl_rl)
            perm = torch.randperm(nmb * mb, device=self.device)
        self._perm_buf.copy_(perm[:nmb * mb])
        return [self._perm_buf[i * mb:(i + 1) * mb] for i in range(nmb)]

    def _steps(self, slots):
        """epochs x mini-batches: every mini-batch slot (its rows, or its graph) once per epoch."""
        return (slot for _ in range(self.num_learning_epochs) for slot in slots)

    def _end_update(self):
        n = self.num_learning_epochs * self.num_mini_batches
        mean_v, mean_s, lr = (float(x) for x in torch.cat((self._acc / n, self._lr.view(1))).cpu())
        self.learning_rate = lr
        self._updates_done += 1
        self.storage.clear()
        return mean_v, mean_s

    def _capturing(self):
        """(graph, context that captures into it on the capture stream)."""
        g = torch.cuda.CUDAGraph()
        return g, torch.cuda.graph(g, stream=self._gstream, capture_error_mode="thread_local")

    def _run_single(self, views):
        """One process: update 0 eager ON THE CAPTURE STREAM -- the warm-up torch asks for before capturing autograd + optimiser work
        (library handles / workspaces and the optimiser state get created on that stream, outside capture) -- capture at update 1,
        replay from then on."""
        cur, gs = torch.cuda.current_stream(self.device), self._gstream
        if self._graph is None and self._updates_done >= 1:
            # On the kernel path a mini-batch step is 5 launches, so all epochs x mini-batches go into ONE graph (each step reading
            # its own slice of _perm_buf); the torch MLP path (~150 launches and fresh activations per step) keeps a one-step graph
            # that reads _ix_one.
            self._graph_whole = self._mlp is not None and self._adam_kernel and (not self._mlp.has_fused_minibatch or self._fused_minibatch)
            gs.wait_stream(cur)
            self._zero_grad()
            g, capture = self._capturing()
            with capture:
                for ix in self._steps(views) if self._graph_whole else [self._ix_one]:
                    self._mb_step(ix)
            self._graph = g                          # (the capture did not execute: this update replays it like every later one)
        if self._graph is None:
            for ix in self._steps(views):
                gs.wait_stream(cur)
                with torch.cuda.stream(gs):
                    self._zero_grad()
                    self._mb_step(ix)
                cur.wait_stream(gs)
        elif self._graph_whole:
            self._graph.replay()
        else:
            for ix in self._steps(views):
                self._ix_one.copy_(ix)
                self._graph.replay()

    def _run_data_parallel(self, views):
        """world_size > 1, loss kernel path.  A mini-batch step is [backward graph] -> flat all-reduce (RCCL, eager: one collective of all
        gradients + the KL slot) -> [optimiser graph]: after an eager first update the two halves are captured once -- one "pre" graph
        per mini-batch slot (``_gradients`` on its own slice of the permutation buffer), one "post" graph (``_optimise``) -- so an update
        is 2 x epochs x mini-batches graph replays + epochs x mini-batches collectives from the host, no kernel launch of its own."""
        self.dp_launches = None
        if self._dp_graphs_wanted and self._mlp_kernels and self._adam_kernel and self._updates_done >= 1 and self._dp_graphs is None:
            try:
                if self._mlp_trainer(views[0].numel()) is None:
                    raise RuntimeError("no learner kernels for these networks")
                self._gstream.wait_stream(torch.cuda.current_stream(self.device))
                pre_graphs = []
                for ix in views:
                    g, capture = self._capturing()
                    with capture:
                        self._zero_grad()
                        flat, acc_done = self._gradients(ix)
                        if not flat:
                            raise RuntimeError("the two-graph data-parallel step needs the flat-gradient kernel path")
                    pre_graphs.append(g)
                post, capture = self._capturing()
                with capture:
                    self._optimise(True, acc_done)   # (the same for every slot: known here, at capture time)
                self._dp_graphs, self._dp_graph_error = (pre_graphs, post), None
            except Exception as exc:                  # capture refused (e.g. the torch MLP path): stay eager, say so once
                self._dp_graphs = False
                self._dp_graph_error = f"{type(exc).__name__}: {exc}"
        if self._dp_graphs:
            pre_graphs, post = self._dp_graphs
            for pre in self._steps(pre_graphs):
                pre.replay()
                self._collective(True)
                post.replay()
            n = self.num_learning_epochs * self.num_mini_batches
            self.dp_launches = {"graph_replays": 2 * n, "collectives": n, "kernel_launches_from_host": 0}
        else:
            for ix in self._steps(views):
                self._zero_grad()
                self._mb_step(ix)

    def update(self, perm=None):
        """One PPO update over the stored rollout.  ``perm`` (optional) fixes the mini-batch permutation (tests)."""
        if self._graph_ok and (_world() == 1 or self._fused_ready()):
            views = self._begin_update(perm)
            if _world() == 1:
                self._run_single(views)
            else:
                self._run_data_parallel(views)
            return self._end_update()
        mean_v, mean_s = 0.0, 0.0
        if self.actor_critic.is_recurrent:
            gen = self.storage.recurrent_mini_batch_generator(self.num_mini_batches, self.num_learning_epochs)
        else:
            gen = self.storage.mini_batch_generator(self.num_mini_batches, self.num_learning_epochs, perm)
        for obs, cobs, act, tval, adv, ret, old_lp, old_mu, old_sig, hid, masks in gen:
            self.actor_critic.act(obs, masks=masks, hidden_states=hid[0])
            lp = self.actor_critic.get_actions_log_prob(act)
            val = self.actor_critic.evaluate(cobs, masks=masks, hidden_states=hid[1])
            mu, sig, ent = self.actor_critic.action_mean, self.actor_critic.action_std, self.actor_critic.entropy
            if self._adaptive:
                with torch.inference_mode():
                    kl_mean = gaussian_kl(mu, sig, old_mu, old_sig).mean()
                    if _world() > 1:
                        dist.all_reduce(kl_mean, op=dist.ReduceOp.SUM)
                        kl_mean /= _world()
                    if kl_mean > self.desired_kl * 2.0:
                        self.learning_rate = max(1e-5, self.learning_rate / 1.5)
                    elif 0.0 < kl_mean < self.desired_kl / 2.0:
                        self.learning_rate = min(1e-2, self.learning_rate * 1.5)
                    for g in self.optimizer.param_groups:
                        g["lr"] = self.learning_rate
            loss, surrogate, vloss = self._loss(lp, old_lp.squeeze(-1), adv.squeeze(-1), val, tval, ret, ent)
            self.optimizer.zero_grad()
            loss.backward()
            self._allreduce_grads()
            nn.utils.clip_grad_norm_(self.actor_critic.parameters(), self.max_grad_norm)
            self.optimizer.step()
            mean_v += vloss.item()
            mean_s += surrogate.item()
        n = self.num_learning_epochs * self.num_mini_batches
        self.storage.clear()
        return mean_v / n, mean_s / n
