"""The table digests' definitions (include/p2pmg.h) on the host: the NumPy reference on hand-written
rows, and the unbound QActor's greedy_policy() / table_stats() against that reference."""
import numpy as np

import table_digest_ref as ref


def test_reference_on_hand_written_rows():
    q = np.array([[
        [1.0, 2.0, 2.0],      # tie between actions 1 and 2: the first maximum wins
        [0.0, 0.0, 0.0],      # all zero: unvisited, greedy action 0
        [-0.0, -0.0, -0.0],   # only -0.0: still unvisited
        [-3.0, -1.0, -2.0],   # all negative: action 1, visited
        [0.0, 0.0, 5e-324],   # a single non-zero entry (the smallest denormal): visited, action 2
        [0.0, -7.0, 0.0],     # a single negative entry: visited, the tie of zeros goes to action 0
        [4.0, 4.0, 4.0],      # three-way tie: action 0
    ]])
    assert ref.visited(q).tolist() == [[True, False, False, True, True, True, True]]
    assert ref.greedy(q).tolist() == [[1, 0, 0, 1, 2, 0, 0]]
    assert ref.policy(q).tolist() == [[1, 255, 255, 1, 2, 0, 0]]
    s = ref.stats(q)
    assert s["visited"].tolist() == [5] and s["greedy"].tolist() == [[2, 2, 1]]
    assert (s["q_min"][0], s["q_max"][0], s["abs_max"][0]) == (-7.0, 4.0, 7.0)
    assert s["visited"].dtype == np.int64 and s["greedy"].dtype == np.int64


def test_reference_zero_extrema_are_positive_zero():
    q = np.array([[[-0.0, 0.0], [0.0, -0.0]], [[-0.0, -0.0], [-0.0, -0.0]], [[-0.0, -2.0], [-0.0, -1.0]]])
    s = ref.stats(q)
    assert s["visited"].tolist() == [0, 0, 2] and s["greedy"].tolist() == [[0, 0], [0, 0], [2, 0]]
    assert s["q_max"].tolist() == [0.0, 0.0, 0.0] and not np.signbit(s["q_max"]).any()
    assert not np.signbit(s["q_min"][:2]).any() and not np.signbit(s["abs_max"][:2]).any()
    assert s["q_min"][2] == -2.0 and s["abs_max"][2] == 2.0


def test_reference_changes():
    old = np.array([[255, 0, 1, 255, 2, 255]], np.uint8)
    new = np.array([[0, 1, 1, 2, 255, 255]], np.uint8)
    # 255 -> 0: newly visited, not changed; 0 -> 1: changed; 255 -> 2: both; 2 -> 255: changed (2 -> 0)
    changed, newly = ref.changes(old, new)
    assert changed.tolist() == [3] and newly.tolist() == [2]


def _actor(shape, na):
    from p2pmicrogrid_amd.rl import QActor
    return QActor(*shape, num_actions=na)


def test_unbound_qactor_matches_reference():
    """An actor that is not on a device answers from its NumPy table by the same definitions."""
    rs = np.random.RandomState(5)
    for shape, na in (((3, 4, 5, 2), 3), ((3, 4, 5, 2), 2), ((4, 3, 2, 5), 4)):
        n = int(np.prod(shape))
        q = rs.standard_normal((n, na))
        q[rs.rand(n) < 0.33] = 0.0
        q[1] = q[1, 0]                 # ties
        q[2, :2] = np.abs(q[2]).max() + 1.0
        q[3] = -0.0
        q[4] = -np.abs(q[4]) - 1.0     # all negative
        actor = _actor(shape, na)
        fresh_pol, fresh = actor.greedy_policy(), actor.table_stats()
        assert fresh_pol.shape == shape and fresh_pol.dtype == np.uint8 and (fresh_pol == 255).all()
        ref.assert_stats_equal({k: np.asarray(v)[None] for k, v in fresh.items()},
                               ref.stats(np.zeros((1, n, na))), "fresh")
        actor.set_qtable(q.reshape(*shape, na))
        assert actor._engine is None  # still unbound: nothing touched a device
        pol = actor.greedy_policy()
        assert pol.shape == shape and pol.dtype == np.uint8
        assert np.array_equal(pol.reshape(1, n), ref.policy(q[None]))
        ref.assert_stats_equal({k: np.asarray(v)[None] for k, v in actor.table_stats().items()},
                               ref.stats(q[None]), f"{shape} x {na}")
