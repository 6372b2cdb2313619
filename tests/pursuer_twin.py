"""NumPy float32 restatement of k_pursuer_post (csrc/lg_pursuer_game.hip) on top of tests/game_twin.py: the scripted pursuer's velocity
(reference high_level_game.py:297-315 with ``command=None``), then ``game_twin.post`` with that velocity in columns 4:6 of the command.

    ep  = curr_episode_step + 1
    dxy = (prey_xy - predator_xy) * gain
    a   = (L - ep) / L
    lim = min_lin_vel * (1 - a) + max_lin_vel * a
    v   = min(max(dxy, -lim), lim)             # torch.clamp: lim < 0 (ep > L) gives v = lim

Every operation rounds once, in float32, in this order; NumPy's float32 division is correctly rounded, as torch's is."""
import numpy as np

from tests import game_twin as tw

F = np.float32


def pursuer_params(**kw):
    """The fields of lg_pursuer_params with the registered task's values; keyword arguments override."""
    q = dict(max_lin_vel=2.0, min_lin_vel=0.01, gain=2.0, max_episode_length=1000)
    q.update(kw)
    return q


def speed_limit(q, ep):
    """``lim`` [N] for the post-increment episode step ``ep`` (any integer array)."""
    L = F(q["max_episode_length"])
    a = ((L - np.asarray(ep).astype(F)).astype(F) / L).astype(F)
    return ((F(q["min_lin_vel"]) * (F(1) - a).astype(F)).astype(F) + (F(q["max_lin_vel"]) * a).astype(F)).astype(F)


def velocity(q, prey_xy, predator_xy, ep):
    """-> (v [N,2], lim [N])."""
    lim = speed_limit(q, ep)
    dxy = ((np.asarray(prey_xy, F) - np.asarray(predator_xy, F)).astype(F) * F(q["gain"])).astype(F)
    return np.minimum(np.maximum(dxy, -lim[:, None]), lim[:, None]).astype(F), lim


def post(p, q, s, step=None, u_root=None, u_pred=None):
    """k_pursuer_post on a ``game_twin.post`` state dict (columns 4:6 of its ``command`` are ignored) -> (new state dict, info dict);
    info gains ``predator_command`` [N,2], ``lim`` [N] and ``ep`` [N], the step count the limit was computed from."""
    ep = s["curr_episode_step"] + 1
    v, lim = velocity(q, s["root_states"][:, :2], s["predator_pos"][:, :2], ep)
    command = np.array(s["command"], F, copy=True)
    command[:, 4:6] = v
    out, info = tw.post(p, dict(s, command=command), step=step, u_root=u_root, u_pred=u_pred)
    out["command"] = np.array(s["command"], copy=True)
    info.update(predator_command=v, lim=lim, ep=ep)
    return out, info


def branch_shares(info):
    """(share of unsaturated velocity components, share saturated at a positive limit, share of envs with a negative limit)."""
    v, lim = info["predator_command"], info["lim"][:, None]
    return float(((lim > 0) & (np.abs(v) < lim)).mean()), float(((lim > 0) & (np.abs(v) == lim)).mean()), float((info["lim"] < 0).mean())
