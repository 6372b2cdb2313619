"""The one comparison of an actor kernel's exploration noise with ``tests/philox_np.action_noise``, shared by the rollout-oracle tests and
the recurrent-actor tests.  Tolerances: the kernels use __logf / __sincosf, so the comparison is approximate; a wrong Philox purpose, step,
env or group gives O(1) differences."""
import numpy as np

from tests.philox_np import action_noise

NOISE_MAX, NOISE_MEDIAN = 1e-3, 1e-5


def check_noise(actions, mean, std, seed, step, report, env_ids=None):
    """``actions - mean`` [N, n] is ``std * eps`` of the reference for (seed; env, step): every element within ``NOISE_MAX`` of the smallest
    std, the median relative error within ``NOISE_MEDIAN``.  ``env_ids``: the env of every row (0 .. N - 1 when not given)."""
    N, n = actions.shape
    eps = action_noise(seed, np.arange(N) if env_ids is None else env_ids, step, n)
    got = actions.astype(np.float64) - mean.astype(np.float64)
    err = np.abs(got - std * eps)
    assert err.max() <= NOISE_MAX * std.min(), (float(err.max()), np.unravel_index(err.argmax(), err.shape))
    rel = float(np.median(err / (std * (1.0 + np.abs(eps)))))
    assert rel <= NOISE_MEDIAN, rel
    report["noise_max"] = max(report.get("noise_max", 0.0), float((err / std).max()))
    report["noise_median"] = max(report.get("noise_median", 0.0), rel)
