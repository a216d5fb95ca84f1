"""NumPy reference of the DQN policy map (p2pmg_dqn_policy_map & co.): a helper, not a test.

The Q values are oracle.dqn.act_q's (the act kernels' summation order, bit for bit) at the grid's
observations in grid order; the greedy action, the eight stats and the change counts are plain NumPy.
"""
import numpy as np

from oracle import dqn as odqn

F32 = np.float32
STAT_KEYS = ("states", "q_min", "q_max", "abs_max", "greedy", "min_gap")


def default_axes(shape):
    """The default grid of a context with table shape (n_time, n_temp, n_balance, n_p2p): each axis at its
    bins' centres, formed in f64 and cast to f32 (include/p2pmg.h)."""
    kt, kT, kb, kp = (int(k) for k in shape)
    k = lambda n: np.arange(n, dtype=np.float64)  # noqa: E731
    return (((k(kt) + 0.5) / kt).astype(F32), (2.0 * (k(kT) - 0.5) / (kT - 2) - 1.0).astype(F32),
            (2.0 * (k(kb) + 0.5) / kb - 1.0).astype(F32), (2.0 * (k(kp) + 0.5) / kp - 1.0).astype(F32))


def grid_obs(axes):
    """[G, 4] f32 observations in state order g = ((i0 n1 + i1) n2 + i2) n3 + i3."""
    ax = [np.asarray(a, F32).reshape(-1) for a in axes]
    return np.stack([m.reshape(-1) for m in np.meshgrid(*ax, indexing="ij")], axis=-1).astype(F32)


def argmax_first(q):
    """g = 0; for k = 1, 2: if q[k] > q[g] then g = k (rl.py:188-196: the first maximum)."""
    q = np.asarray(q, F32)
    g = np.zeros(q.shape[:-1], np.uint8)
    best = q[..., 0].copy()
    for k in (1, 2):
        up = q[..., k] > best
        g[up] = k
        best = np.where(up, q[..., k], best)
    return g


def fold_stats(q, policy):
    """The eight stats of one network from its Q values [..., 3] and policy [...] (DeviceDQNBatch.map_stats'
    keys, scalars and a [3] histogram)."""
    q = np.asarray(q, F32).reshape(-1, 3)
    pol = np.asarray(policy).reshape(-1).astype(np.int64)
    rows = np.arange(len(q))
    best = q[rows, pol]
    others = np.where(np.arange(3)[None, :] == pol[:, None], F32(-np.inf), q).max(axis=1)
    gap = (best - others).astype(F32)  # one f32 subtraction per state
    lo, hi = np.float64(q.min()), np.float64(q.max())
    return {"states": np.int64(len(q)), "q_min": lo + 0.0, "q_max": hi + 0.0, "abs_max": max(-lo, hi) + 0.0,
            "greedy": np.bincount(pol, minlength=3).astype(np.int64), "min_gap": np.float64(gap.min()) + 0.0}


def map_ref(theta, axes, chunk=4096):
    """(policy u8 [n0, n1, n2, n3], q f32 [n0, n1, n2, n3, 3], stats dict) of one network theta [4609]."""
    obs = grid_obs(axes)
    q = np.concatenate([odqn.act_q(theta, obs[k:k + chunk]) for k in range(0, len(obs), chunk)]).astype(F32)
    shape = tuple(len(np.asarray(a).reshape(-1)) for a in axes)
    pol = argmax_first(q)
    return pol.reshape(shape), q.reshape(shape + (3,)), fold_stats(q, pol)


def changes(policy, snapshot):
    """Number of states whose greedy action differs from the snapshot's."""
    return np.int64(np.count_nonzero(np.asarray(policy) != np.asarray(snapshot)))


def same_bits(a, b):
    """array_equal on the bit patterns (tells +0.0 from -0.0)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
