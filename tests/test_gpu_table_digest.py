"""Table digests on the device (p2pmg_table_stats, p2pmg_greedy_policy, p2pmg_policy_mark,
p2pmg_policy_changes).  The expected values always come from tests/table_digest_ref.py applied to what
get_q() returns, and every comparison is bit for bit.

Shapes: 3 x 4 x 5 x 2 = 120 states (not a multiple of 64, less than one block), the same with 2 actions,
3 x 3 x 3 x 3 = 81 states (odd: the policy bytes of tables 1, 2, ... start unaligned, the byte-store
form) and the reference's 20^4 = 160000 states with 3 tables (157 blocks per table, the last one a
256-row tail), each in f64 and f32."""
import numpy as np
import pytest

import table_digest_ref as ref

pytestmark = pytest.mark.gpu

SMALL = dict(n_time_states=3, n_temp_states=4, n_balance_states=5, n_p2p_states=2)
ODD = dict(n_time_states=3, n_temp_states=3, n_balance_states=3, n_p2p_states=3)
FULL = {}  # the config's 20 x 20 x 20 x 20


def _engine(S=2, N=3, q="f64", shared=False, T=1, R=0, **cfg):
    from p2pmicrogrid_amd.engine import DeviceCommunityBatch
    return DeviceCommunityBatch(S, N, R, T, q_dtype=q, shared_q=shared, **cfg)


def _tables(n_tables, n_states, na, q, seed=3):
    """[n_tables, n_states, na] in the context's element type: random normals with about a third of the
    rows zero, then ties at every action pair (the tie the maximum, and the tie below a third entry), rows
    of +-0.0, huge / tiny / denormal magnitudes and all-negative rows at scattered places; table 1 (where
    there is one) is entirely zero."""
    dt = np.float64 if q == "f64" else np.float32
    fi = np.finfo(dt)
    rs = np.random.RandomState(seed)
    t = rs.standard_normal((n_tables, n_states, na)).astype(dt)
    t[rs.rand(n_tables, n_states) < 0.33] = 0
    special = []
    for i in range(na):
        for j in range(i + 1, na):
            hi_tie = np.full(na, -1.5, dt)
            hi_tie[[i, j]] = 2.5
            lo_tie = np.full(na, 3.5, dt)
            lo_tie[[i, j]] = -2.5
            neg_tie = np.full(na, -9.0, dt)
            neg_tie[[i, j]] = -0.25
            special += [hi_tie, lo_tie, neg_tie]
    special += [np.full(na, -0.0, dt), np.array([0.0, -0.0, 0.0, -0.0][:na], dt), np.full(na, 7.0, dt)]
    for k in range(na):
        for v in (fi.max, -fi.max, fi.tiny, -fi.tiny, fi.smallest_subnormal, -fi.smallest_subnormal):
            row = np.zeros(na, dt)
            row[k] = v
            special.append(row)
        row = np.full(na, -fi.max, dt)
        row[k] = -fi.tiny
        special.append(row)
    special = np.stack(special)
    for a in range(n_tables):
        where = rs.permutation(n_states)[:len(special)]
        t[a, where] = special[:len(where)]
        t[a, -1] = special[a % len(special)]  # the last row of every table: the tail lane of the last wave
    if n_tables > 1:
        t[1] = 0
    return t


def _check(eng, first=0, count=None, tag=""):
    q = eng.get_q(first, count)
    q = q.reshape(q.shape[0], -1, q.shape[-1])
    ref.assert_stats_equal(eng.table_stats(first, count), ref.stats(q), tag)
    pol = eng.greedy_policy(first, count)
    assert pol.dtype == np.uint8 and pol.shape == (q.shape[0], *eng.q_shape[:-1]), (tag, pol.shape)
    want = ref.policy(q)
    assert np.array_equal(pol.reshape(want.shape), want), (tag, np.argwhere(pol.reshape(want.shape) != want)[:5])
    return pol


def _ranges(n):
    """everything, the first table, the last, and a middle pair"""
    r = [(0, None), (0, 1), (n - 1, 1)]
    if n >= 3:
        r.append(((n - 2) // 2, 2))
    return r


@pytest.mark.parametrize("q", ["f64", "f32"])
@pytest.mark.parametrize("shared,n_tables", [(False, 6), (True, 1), ("role", 3)])
@pytest.mark.parametrize("shape,na", [(SMALL, 3), (SMALL, 2), (ODD, 3)], ids=["120x3", "120x2", "81x3"])
def test_small_tables_every_mode_and_range(shape, na, shared, n_tables, q):
    eng = _engine(2, 3, q, shared, n_actions=na, **shape)
    assert eng.n_tables == n_tables and eng.q_shape[-1] == na
    _check(eng, tag="fresh")  # all zero
    eng.set_q(_tables(n_tables, eng.n_states, na, q))
    for first, count in _ranges(n_tables):
        _check(eng, first, count, tag=f"{first}+{count}")
    st = eng.table_stats()
    assert st["greedy"].shape == (n_tables, na) and np.array_equal(st["greedy"].sum(axis=1), st["visited"])
    eng.zero_q()
    assert not eng.table_stats()["visited"].any() and (eng.greedy_policy() == 255).all()


@pytest.mark.parametrize("q", ["f64", "f32"])
def test_full_size_tables_many_blocks_with_a_tail(q):
    eng = _engine(1, 3, q, **FULL)
    assert eng.n_states == 160000
    eng.set_q(_tables(3, eng.n_states, 3, q, seed=11))
    for first, count in _ranges(3):
        _check(eng, first, count, tag=f"{first}+{count}")


def test_two_action_context_holds_tables_but_runs_no_episode():
    from p2pmicrogrid_amd import _lib
    eng = _engine(1, 2, n_actions=2, **SMALL)
    with pytest.raises(_lib.P2PMGError, match="UNSUPPORTED"):
        eng.run_episode("greedy")
    with pytest.raises(_lib.P2PMGError, match="UNSUPPORTED"):
        eng.q_calls([0], np.zeros((1, 4), np.float32), [255])


def test_tables_after_real_training_episodes():
    """Two Philox training episodes at N = 2, R = 1, T = 96 (the fast kernel) leave sparsely written
    tables; against a mark taken before them, every visited row is newly visited."""
    from p2pmicrogrid_amd.dataset import scenario_batch
    S, N, T = 2, 2, 96
    inp = scenario_batch(S, N, T, seed=61)
    eng = _engine(S, N, "f64", T=T, R=1)
    eng.set_env(np.broadcast_to(inp.time, inp.t_out.shape), inp.t_out)
    eng.set_profiles(inp.load_w, inp.pv_w)
    eng.set_max_in(inp.max_in)
    eng.set_temperatures(inp.t_in0, inp.t_m0)
    eng.policy_mark()
    for e in range(2):
        eng.run_episode("train", "philox", episode=e, epsilon=0.5, reset_sigma=0.3)
    pol = _check(eng, tag="trained")
    st = eng.table_stats()
    assert (st["visited"] > 0).all() and (st["visited"] <= 2 * 2 * T).all()
    ch = eng.policy_changes(remark=False)
    want = ref.changes(np.full_like(pol, 255), pol)
    assert np.array_equal(ch["changed"], want[0]) and np.array_equal(ch["newly_visited"], want[1])
    assert np.array_equal(ch["newly_visited"], st["visited"])


def test_shared_table_digest_ignores_the_pending_delta():
    eng = _engine(2, 3, "f64", True, **SMALL)
    t = np.random.RandomState(2).standard_normal((1, eng.n_states, 3))
    t[0, ::3] = 0.0
    eng.set_q(t)
    before = eng.greedy_policy()
    d = np.zeros(eng.q_shape, np.int64)
    d[..., 2] = 1 << 50  # + 1024 on action 2 of every row once applied
    eng.set_q_delta(d)
    assert np.array_equal(_check(eng, tag="pending"), before)
    eng.apply_q_delta()
    assert (_check(eng, tag="applied") == 2).all()


@pytest.mark.parametrize("shape,S,N,q", [(SMALL, 2, 3, "f64"), (ODD, 2, 3, "f32"), (FULL, 1, 3, "f32"), (FULL, 1, 3, "f64")],
                         ids=["120-f64", "81-f32", "160000-f32", "160000-f64"])
def test_policy_churn(shape, S, N, q):
    from p2pmicrogrid_amd import _lib
    eng = _engine(S, N, q, **shape)
    n, ns = eng.n_tables, eng.n_states
    with pytest.raises(_lib.P2PMGError, match="STATE"):
        eng.policy_changes()
    t = _tables(n, ns, 3, q, seed=23)
    eng.set_q(t)
    eng.policy_mark()
    zero = eng.policy_changes(remark=False)
    assert not zero["changed"].any() and not zero["newly_visited"].any()
    old = eng.greedy_policy()
    # known edits: flip the greedy action of visited rows, visit unvisited rows with action 0 the maximum
    # (newly visited, not changed) and with action 2 (both); tables 0 and n - 1, table 1 stays all zero
    flat = old.reshape(n, ns)
    for a, k_flip, k_v0, k_v2 in ((0, 5, 3, 4), (n - 1, 2, 6, 1)):
        vis = np.flatnonzero(flat[a] != 255)
        unv = np.flatnonzero(flat[a] == 255)
        for r in vis[:k_flip]:
            t[a, r] = -1.0
            t[a, r, (int(flat[a, r]) + 1) % 3] = 1.0
        t[a, unv[:k_v0]] = [1.0, 0.5, -1.0]
        t[a, unv[k_v0:k_v0 + k_v2]] = [-1.0, 0.0, 0.25]
        t[a, ns - 1] = [0.0, 0.0, 0.0] if flat[a, ns - 1] != 255 else [0.0, 3.0, 0.0]  # the last row too
    eng.set_q(t)  # set_q leaves the snapshot alone
    new = eng.greedy_policy()
    want = ref.changes(old, new)
    assert want[0][0] >= 5 + 4 and want[1][0] == 3 + 4 + (flat[0, ns - 1] == 255)
    for _ in range(2):  # without remark the second call reports the same numbers
        got = eng.policy_changes(remark=False)
        assert got["changed"].dtype == np.int64 and got["newly_visited"].dtype == np.int64
        assert np.array_equal(got["changed"], want[0]) and np.array_equal(got["newly_visited"], want[1])
    sub = eng.policy_changes(n - 1, 1, remark=True)  # reports, then re-marks the last table only
    assert sub["changed"][0] == want[0][-1] and sub["newly_visited"][0] == want[1][-1]
    after = eng.policy_changes(remark=False)
    assert after["changed"][-1] == 0 and after["newly_visited"][-1] == 0
    assert np.array_equal(after["changed"][:-1], want[0][:-1])
    assert np.array_equal(after["newly_visited"][:-1], want[1][:-1])
    eng.zero_q()  # zero_q leaves the snapshot alone as well: against it, everything visited went back
    back = eng.policy_changes()
    assert not back["newly_visited"].any()
    assert np.array_equal(back["changed"][-1:], ref.changes(new[-1:], np.full_like(new[-1:], 255))[0])
    assert np.array_equal(back["changed"][:-1], ref.changes(old[:-1], np.full_like(old[:-1], 255))[0])
    final = eng.policy_changes()
    assert not final["changed"].any() and not final["newly_visited"].any()


def test_errors():
    from p2pmicrogrid_amd import _lib
    eng = _engine(2, 3, **SMALL)
    for bad in ((5, 2), (-1, 1), (0, 7), (0, -1)):
        with pytest.raises(_lib.P2PMGError, match="INVALID"):
            eng.table_stats(*bad)
        with pytest.raises(_lib.P2PMGError, match="INVALID"):
            eng.greedy_policy(*bad)
    eng.policy_mark()
    with pytest.raises(_lib.P2PMGError, match="INVALID"):
        eng.policy_changes(5, 2)
    # count == 0: OK, nothing written (not even looked at: null outputs)
    assert eng.L.p2pmg_table_stats(eng._ctx, 6, 0, None) == 0
    assert eng.L.p2pmg_greedy_policy(eng._ctx, 0, 0, None) == 0
    assert eng.L.p2pmg_policy_changes(eng._ctx, 3, 0, None, None, 1) == 0
    assert eng.table_stats(2, 0)["visited"].shape == (0,) and eng.greedy_policy(2, 0).shape == (0, 3, 4, 5, 2)
    # a null output with count > 0; newly_visited alone may be null
    assert eng.L.p2pmg_table_stats(eng._ctx, 0, 1, None) == 1
    assert eng.L.p2pmg_greedy_policy(eng._ctx, 0, 1, None) == 1
    assert eng.L.p2pmg_policy_changes(eng._ctx, 0, 1, None, None, 0) == 1
    ch = np.full(6, -1, np.int64)
    assert eng.L.p2pmg_policy_changes(eng._ctx, 0, 6, ch.ctypes.data, None, 0) == 0 and not ch.any()
    # a DQN context has no Q-table
    dqn = _engine(1, 1, "f32", learner=_lib.LEARNER_DQN)
    for call in (dqn.table_stats, dqn.greedy_policy, dqn.policy_mark, dqn.policy_changes):
        with pytest.raises(_lib.P2PMGError, match="STATE.*no Q-table"):
            call()


def test_object_api():
    """A bound QActor asks the device for its slot; CommunityMicrogrid.table_stats() is one pass over the
    community's tables."""
    from p2pmicrogrid_amd.rl import QActor
    rs = np.random.RandomState(9)
    actor = QActor(3, 4, 5, 2)
    q = rs.standard_normal((3, 4, 5, 2, 3))
    q[rs.rand(3, 4, 5, 2) < 0.4] = 0.0
    q[0, 0, 0, 0] = 1.25  # a three-way tie
    actor.set_qtable(q)
    actor._device()  # binds to a private one-agent context
    assert actor._engine is not None
    tab = actor.q_table.reshape(1, -1, 3)
    assert np.array_equal(actor.greedy_policy().reshape(1, -1), ref.policy(tab))
    assert actor.greedy_policy().shape == (3, 4, 5, 2)
    ref.assert_stats_equal({k: np.asarray(v)[None] for k, v in actor.table_stats().items()}, ref.stats(tab), "actor")

    from p2pmicrogrid_amd import community, setup
    from p2pmicrogrid_amd.agent import QAgent
    setup.homogeneous = True  # HPHeating reads the module flag (heating.py:101,149)
    try:
        np.random.seed(42)
        com = community.get_community(QAgent, 2, homogeneous=True)
        before = com.table_stats()  # no engine yet: the unbound actors answer
        assert before["visited"].tolist() == [0, 0] and before["greedy"].shape == (2, 3)
        com.train_episode()
        got = com.table_stats()
        tabs = np.stack([a.actor.q_table for a in com.agents]).reshape(2, -1, 3)
        ref.assert_stats_equal(got, ref.stats(tabs), "community")
        assert (got["visited"] > 0).all()
    finally:
        setup.homogeneous = False
