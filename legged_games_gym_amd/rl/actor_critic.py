"""Gaussian MLP actor + MLP critic (hyper-parameters: reference
``legged_robot_config.py:204-213``, flat override ``anymal_c_flat_config.py:62-65``)."""
import torch
import torch.nn as nn
from torch.distributions import Normal

_ACT = {"elu": nn.ELU, "relu": nn.ReLU, "selu": nn.SELU, "lrelu": nn.LeakyReLU, "tanh": nn.Tanh, "sigmoid": nn.Sigmoid}


def _mlp(n_in, hidden, n_out, act):
    layers, last = [], n_in
    for h in hidden:
        layers += [nn.Linear(last, h), _ACT[act]()]
        last = h
    layers.append(nn.Linear(last, n_out))
    return nn.Sequential(*layers)


class ActorCritic(nn.Module):
    is_recurrent = False

    def __init__(self, num_actor_obs, num_critic_obs, num_actions, actor_hidden_dims=(256, 256, 256),
                 critic_hidden_dims=(256, 256, 256), activation="elu", init_noise_std=1.0, **kwargs):
        super().__init__()
        if kwargs:
            print("ActorCritic.__init__ got unexpected arguments, which will be ignored: " + str(list(kwargs.keys())))
        self.actor = _mlp(num_actor_obs, list(actor_hidden_dims), num_actions, activation)
        self.critic = _mlp(num_critic_obs, list(critic_hidden_dims), 1, activation)
        self.std = nn.Parameter(init_noise_std * torch.ones(num_actions))
        self.distribution = None
        Normal.set_default_validate_args(False)     # no host-syncing argument checks (also keeps act() graph-capturable)

    def reset(self, dones=None):
        pass

    @property
    def action_mean(self):
        return self.distribution.mean

    @property
    def action_std(self):
        return self.distribution.stddev

    @property
    def entropy(self):
        return self.distribution.entropy().sum(dim=-1)

    def update_distribution(self, observations):
        mean = self.actor(observations)
        self.distribution = Normal(mean, mean * 0.0 + self.std)

    def act(self, observations, **kwargs):
        self.update_distribution(observations)
        # == self.distribution.sample(), written without torch.normal(tensor, tensor), whose std >= 0 check
        # synchronises with the host (and therefore cannot be captured into a HIP graph)
        mean = self.distribution.mean
        return mean + self.distribution.stddev * torch.randn_like(mean)

    def get_actions_log_prob(self, actions):
        return self.distribution.log_prob(actions).sum(dim=-1)

    def act_inference(self, observations):
        return self.actor(observations)

    def evaluate(self, critic_observations, **kwargs):
        return self.critic(critic_observations)


def split_and_pad_trajectories(tensor, dones):
    """Cut ``tensor`` [T, N, ...] after every done (and after the last step) and stack the pieces env-major, each padded with zeros
    to T: ``([T, n_traj, ...], masks [T, n_traj])`` with ``masks[t, j]`` true where trajectory ``j`` has a step ``t`` (rsl_rl's
    function of the same name, which pads to the longest piece only)."""
    T = tensor.shape[0]
    dones = dones.reshape(T, -1).clone()
    dones[-1] = 1
    flat = dones.transpose(1, 0).reshape(-1)
    ends = torch.cat((flat.new_tensor([-1], dtype=torch.int64), flat.nonzero(as_tuple=False)[:, 0]))
    lengths = ends[1:] - ends[:-1]
    steps = torch.arange(T, device=tensor.device).unsqueeze(1)
    masks = lengths.unsqueeze(0) > steps                                        # [T, n_traj]
    padded = tensor.new_zeros((T, lengths.numel()) + tuple(tensor.shape[2:]))
    padded.transpose(1, 0)[masks.transpose(1, 0)] = tensor.transpose(1, 0).flatten(0, 1)
    return padded, masks


def unpad_trajectories(trajectories, masks):
    """Inverse of ``split_and_pad_trajectories``: [T, n_traj, F] -> [T, N, F]."""
    T = trajectories.shape[0]
    return trajectories.transpose(1, 0)[masks.transpose(1, 0)].view(-1, T, trajectories.shape[-1]).transpose(1, 0)


class Memory(nn.Module):
    """One recurrent network (sequence-first ``nn.LSTM`` / ``nn.GRU``) and the state it carries between rollout steps."""

    def __init__(self, input_size, type="lstm", num_layers=1, hidden_size=256):
        super().__init__()
        kind = str(type).lower()
        if kind not in ("lstm", "gru"):
            raise ValueError(f"rnn_type must be 'lstm' or 'gru', got {type!r}")
        self.rnn = (nn.GRU if kind == "gru" else nn.LSTM)(input_size=input_size, hidden_size=hidden_size, num_layers=num_layers)
        self.hidden_states = None
        self.sequence = None                          # batch mode on the device kernels (rl.lstm_sequence.DeviceLstmSequence, attached by PPO(device_bptt=True)); no sub-module, no parameter

    def forward(self, input, masks=None, hidden_states=None):
        if masks is not None:                         # batch mode (policy update): padded trajectories from their stored initial states
            if hidden_states is None:
                raise ValueError("Hidden states not passed to memory module during policy update")
            out = self.sequence(input, hidden_states) if self.sequence is not None else self.rnn(input, hidden_states)[0]
            return unpad_trajectories(out, masks)
        self._own_states()
        out, states = self.rnn(input.unsqueeze(0), self.hidden_states)      # rollout mode: one step on the carried state
        # (detached: nothing trains through the rollout, and a caller outside no_grad would otherwise grow the graph step by step)
        self.hidden_states = tuple(s.detach() for s in states) if isinstance(states, tuple) else states.detach()
        return out

    def _own_states(self):
        """A state left behind by a rollout under inference_mode can neither enter an autograd-recording call nor be written in place
        outside inference_mode: replace it by a copy there."""
        carried = self.hidden_states
        if carried is None or torch.is_inference_mode_enabled():
            return
        fix = lambda s: s.clone() if s.is_inference() else s
        self.hidden_states = tuple(fix(s) for s in carried) if isinstance(carried, tuple) else fix(carried)

    def reset(self, dones=None):
        if self.hidden_states is None:
            return
        self._own_states()
        states = self.hidden_states if isinstance(self.hidden_states, tuple) else (self.hidden_states,)
        for s in states:
            if dones is None:
                s.zero_()
            else:                                     # (a product, not an index: no host sync, any flag dtype)
                s.mul_((dones.reshape(1, -1, 1) == 0).to(device=s.device, dtype=s.dtype))


class ActorCriticRecurrent(ActorCritic):
    """``ActorCritic`` whose actor and critic each read the output of a ``Memory`` of their own (rsl_rl's class of the same name,
    parameter names included, so checkpoints move between the two)."""
    is_recurrent = True

    def __init__(self, num_actor_obs, num_critic_obs, num_actions, actor_hidden_dims=(256, 256, 256), critic_hidden_dims=(256, 256, 256),
                 activation="elu", rnn_type="lstm", rnn_hidden_size=256, rnn_num_layers=1, init_noise_std=1.0, **kwargs):
        if kwargs:
            print("ActorCriticRecurrent.__init__ got unexpected arguments, which will be ignored: " + str(list(kwargs.keys())))
        super().__init__(num_actor_obs=rnn_hidden_size, num_critic_obs=rnn_hidden_size, num_actions=num_actions, actor_hidden_dims=actor_hidden_dims,
                         critic_hidden_dims=critic_hidden_dims, activation=activation, init_noise_std=init_noise_std)
        self.memory_a = Memory(num_actor_obs, type=rnn_type, num_layers=rnn_num_layers, hidden_size=rnn_hidden_size)
        self.memory_c = Memory(num_critic_obs, type=rnn_type, num_layers=rnn_num_layers, hidden_size=rnn_hidden_size)

    def reset(self, dones=None):
        self.memory_a.reset(dones)
        self.memory_c.reset(dones)

    def act(self, observations, masks=None, hidden_states=None):
        return super().act(self.memory_a(observations, masks, hidden_states).squeeze(0))

    def act_inference(self, observations):
        return super().act_inference(self.memory_a(observations).squeeze(0))

    def evaluate(self, critic_observations, masks=None, hidden_states=None):
        return super().evaluate(self.memory_c(critic_observations, masks, hidden_states).squeeze(0))

    def get_hidden_states(self):
        return self.memory_a.hidden_states, self.memory_c.hidden_states
