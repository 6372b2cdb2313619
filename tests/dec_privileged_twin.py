"""NumPy restatement of ``k_privileged_obs`` (csrc/lg_dec_game_privileged.hip, include/legged_dec_game_privileged.h): the critic-only rows of
the decentralised game's two agents from the state the post stage leaves, in float64, with the episode clock also in float32.

Copies and the difference ``p - q`` of two float32 numbers are exact in float64, so their float32 casts are what the device writes, bit for
bit; the clock ``(L - episode_length_buf) / L`` of two small integers is correctly rounded on the device (``game_quotient``) and here (IEEE
division in float32).  ``fx, fy`` sit behind the device's 1-ulp square root and 2.5-ulp division: float64 is their reference, within
``FORWARD_TOL``.  What it needs of the post stage's twin comes from tests/dec_game_twin.py."""
import numpy as np

from tests.dec_game_twin import F, params, post  # noqa: F401  (the post stage whose output state the rows are taken from)

NUM_PRIV_PREY, NUM_PRIV_PRED = 22, 10
# fx, fy against float64: about 4 relative ulp in yz / yw from the square root and the 2.5-ulp division, doubled by the product of magnitude
# <= 2, gives <= 17.5 * 2^-23 ~ 2.1e-6; the bar is that with under 2x slack
FORWARD_TOL = 2.0 ** -18


def forward64(quat):
    """The yaw-forward vector of ``game_observe`` from quaternions [N,4] (x, y, z, w), in float64 on the float32 inputs."""
    z, w = np.asarray(quat, F)[:, 2].astype(np.float64), np.asarray(quat, F)[:, 3].astype(np.float64)
    qn = np.maximum(np.sqrt(z * z + w * w), 1e-9)
    yz, yw = z / qn, w / qn
    tz = yz * 2.0
    return 1.0 - yz * tz, yw * tz


def clock64(p, episode_length_buf):
    L = float(int(p["max_episode_length"]))
    return (L - np.asarray(episode_length_buf).astype(np.float64)) / L


def clock32(p, episode_length_buf):
    """The clock as the device rounds it: one float32 division of two exactly represented integers."""
    L = F(int(p["max_episode_length"]))
    return ((L - np.asarray(episode_length_buf).astype(F)).astype(F) / L).astype(F)


def privileged(p, s):
    """``s``: a state as ``dec_game_twin.post`` returns it (predator_pos, root_states, obs_prey, obs_pred, episode_length_buf) ->
    (prey rows [N,22], predator rows [N,10]) in float64."""
    pp, root = np.asarray(s["predator_pos"], F).astype(np.float64), np.asarray(s["root_states"], F).astype(np.float64)
    oy, op = np.asarray(s["obs_prey"], F).astype(np.float64), np.asarray(s["obs_pred"], F).astype(np.float64)
    n = root.shape[0]
    fx, fy = forward64(s["root_states"][:, 3:7])
    clock = clock64(p, s["episode_length_buf"])
    prey, pred = np.zeros((n, NUM_PRIV_PREY)), np.zeros((n, NUM_PRIV_PRED))
    prey[:, 0:16] = oy
    prey[:, 16:19] = pp - root[:, 0:3]
    prey[:, 19], prey[:, 20], prey[:, 21] = fx, fy, clock
    pred[:, 0:3] = op
    pred[:, 3], pred[:, 4] = fx, fy
    pred[:, 5:8] = root[:, 7:10]
    pred[:, 8] = oy[:, 15]
    pred[:, 9] = clock
    return prey, pred


EXACT_PREY = tuple(range(19)) + (21,)        # columns the device matches bit for bit (with column 21 from clock32)
EXACT_PRED = (0, 1, 2, 5, 6, 7, 8, 9)
FORWARD_PREY, FORWARD_PRED = (19, 20), (3, 4)


def privileged32(p, s):
    """The float32 rows: every exact column is the device's bits; the forward columns are float64 rounded once (a reference, not the bits)."""
    prey, pred = privileged(p, s)
    prey32, pred32 = prey.astype(F), pred.astype(F)
    prey32[:, 21] = pred32[:, 9] = clock32(p, s["episode_length_buf"])
    return prey32, pred32


def check_rows(p, s, got_prey=None, got_pred=None):
    """Device rows against the twin: exact columns bit-equal, ``fx, fy`` within ``FORWARD_TOL`` of float64.  Returns the worst forward error."""
    want_prey64, want_pred64 = privileged(p, s)
    want_prey, want_pred = privileged32(p, s)
    worst = 0.0
    for got, want, want64, exact, forward, who in ((got_prey, want_prey, want_prey64, EXACT_PREY, FORWARD_PREY, "prey"),
                                                    (got_pred, want_pred, want_pred64, EXACT_PRED, FORWARD_PRED, "pred")):
        if got is None:
            continue
        got = np.ascontiguousarray(got, F)
        assert got.shape == want.shape, (who, got.shape)
        for c in exact:
            np.testing.assert_array_equal(got[:, c].view(np.uint32), np.ascontiguousarray(want[:, c]).view(np.uint32), err_msg=f"{who} column {c}")
        err = np.abs(got[:, list(forward)].astype(np.float64) - want64[:, list(forward)])
        worst = max(worst, float(err.max()))
        assert (err <= FORWARD_TOL).all(), (who, float(err.max()))
    return worst


def designed_state(p, n, first=0):
    """``n`` designed envs as the post stage leaves them (its twin runs on them once, with nothing done): row ``first + i`` takes the predator
    dead ahead, dead behind, on both edges of the field of view, inside and outside it (eight bearings), the robot yawed through all four
    quadrants (five yaws), ``episode_length_buf`` through 0, 1, L - 1, L.  Returns (state, visible flags)."""
    k = first + np.arange(n)
    hf = float(p["half_fov"])
    bearing = np.array([0.0, np.pi, hf, -hf, 0.3, -0.3, 1.5, -2.5])[k % 8]
    yaw = np.array([0.4, 2.0, -2.6, -0.9, 3.1])[k % 5]
    dist = 1.0 + 0.37 * (k % 7)
    L = int(p["max_episode_length"])
    root = np.zeros((n, 13), F)
    root[:, 0], root[:, 1], root[:, 2] = 3.0 * (k % 16), 3.0 * (k // 16), 0.30 + 0.01 * (k % 11)
    q = np.stack((0.03 * np.cos(k), 0.03 * np.sin(k), np.sin(yaw / 2), np.cos(yaw / 2)), axis=1)
    root[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    root[:, 7:13] = 0.1 * np.stack([np.sin(k + j) for j in range(6)], axis=1)
    pred = np.stack((root[:, 0] + dist * np.cos(yaw + bearing), root[:, 1] + dist * np.sin(yaw + bearing), np.full(n, 0.3)), axis=1).astype(F)
    obs = np.stack([np.cos(0.7 * k + j) for j in range(16)], axis=1).astype(F)
    obs[:, 12:16] = (k[:, None] + np.arange(4)[None, :]) % 2
    origins = np.zeros((n, 3), F)
    origins[:, :2] = root[:, :2]
    s = dict(predator_pos=pred, obs_prey=obs, dof_pos=np.zeros((n, 12), F), dof_vel=np.zeros((n, 12), F), curr_episode_step=np.full(n, 7, np.int64),
             episode_length_buf=np.full(n, 7, np.int64), episode_sums=np.zeros((3, n), F), episode_means=np.zeros(3, F), env_origins=origins,
             command_prey=np.zeros((n, 4), F), command_pred=np.zeros((n, 2), F), root_states=root, ll_rew=np.zeros(n, F), ll_reset=np.zeros(n, bool))
    out, info = post(dict(p, num_envs=n), s, step=3)
    assert not info["done"].any()
    out["episode_length_buf"] = np.array([0, 1, L - 1, L], np.int64)[k % 4]
    return out, info["visible"]
