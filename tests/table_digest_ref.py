"""The table digests of include/p2pmg.h (p2pmg_table_stats, p2pmg_greedy_policy, p2pmg_policy_changes) in
plain NumPy, on an array q [tables, n_states, n_actions] (padding columns already dropped, as get_q()
returns them).  Written from the header alone; it shares no code with the package.

  visited        any entry of the row != 0 (-0.0 == 0.0)
  greedy action  the first maximum of the row (np.argmax returns the first of equal maxima; NaN-free)
  policy byte    greedy action if visited else 255
"""
import numpy as np

UNVISITED = 255
STAT_FIELDS = ("visited", "q_min", "q_max", "abs_max")


def visited(q):
    return (np.asarray(q) != 0).any(axis=-1)


def greedy(q):
    return np.argmax(np.asarray(q), axis=-1).astype(np.uint8)


def policy(q):
    """u8 [tables, n_states]"""
    return np.where(visited(q), greedy(q), np.uint8(UNVISITED)).astype(np.uint8)


def stats(q):
    """{"visited": [tables] i64, "q_min", "q_max", "abs_max": [tables] f64, "greedy": [tables, n_actions] i64}.
    f32 tables widen exactly; a zero extremum is +0.0 (x + 0.0) whatever zeros the table holds."""
    q = np.asarray(q, np.float64)
    na = q.shape[-1]
    v, g = visited(q), greedy(q)
    flat = q.reshape(q.shape[0], -1)
    return {"visited": v.sum(axis=1).astype(np.int64),
            "q_min": flat.min(axis=1) + 0.0,
            "q_max": flat.max(axis=1) + 0.0,
            "abs_max": np.abs(flat).max(axis=1) + 0.0,
            "greedy": np.stack([(v & (g == k)).sum(axis=1) for k in range(na)], axis=1).astype(np.int64)}


def changes(old_policy, new_policy):
    """(changed, newly_visited) [tables] i64 from two packed policies [tables, ...]: 255 counts as action
    0 on both sides; newly visited = 255 before and not 255 now."""
    o = np.asarray(old_policy).reshape(len(old_policy), -1)
    n = np.asarray(new_policy).reshape(len(new_policy), -1)
    act = lambda p: np.where(p == UNVISITED, 0, p)  # noqa: E731
    return ((act(o) != act(n)).sum(axis=1).astype(np.int64),
            ((o == UNVISITED) & (n != UNVISITED)).sum(axis=1).astype(np.int64))


def assert_stats_equal(got, want, tag=""):
    """Bit for bit: values, dtypes of the counts, and the sign of zero extrema."""
    assert set(got) == set(want), (tag, sorted(got))
    for k in ("visited", "greedy"):
        assert np.asarray(got[k]).dtype == np.int64, (tag, k, np.asarray(got[k]).dtype)
        assert np.array_equal(got[k], want[k]), (tag, k, got[k], want[k])
    for k in ("q_min", "q_max", "abs_max"):
        g, w = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
        assert np.array_equal(g, w) and np.array_equal(np.signbit(g), np.signbit(w)), (tag, k, g, w)
