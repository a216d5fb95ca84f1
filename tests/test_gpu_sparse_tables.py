"""Sparse table checkpoints on the device (p2pmg_sparse_count, p2pmg_get_q_sparse, p2pmg_set_q_sparse,
p2pmg_copy_q).  The expected sparse form always comes from tests/sparse_table_ref.py applied to what
get_q() returns in the tables' own dtype, and every comparison is bit for bit (on uint views, so that
-0.0 and +0.0 differ).

Shapes: 3 x 4 x 5 x 2 = 120 states (not a multiple of 64, less than one block), the same with 2 actions,
3 x 3 x 3 x 3 = 81 states (odd) and the reference's 20^4 = 160000 states with 3 tables (157 blocks per
table, the last one a 256-row tail; the f64 export is walked in more than one staging run), each in f64
and f32."""
import numpy as np
import pytest

import sparse_table_ref as ref

pytestmark = pytest.mark.gpu

SMALL = dict(n_time_states=3, n_temp_states=4, n_balance_states=5, n_p2p_states=2)
ODD = dict(n_time_states=3, n_temp_states=3, n_balance_states=3, n_p2p_states=3)
FULL = {}  # the config's 20 x 20 x 20 x 20
DT = {"f64": np.float64, "f32": np.float32}
OTHER = {"f64": np.float32, "f32": np.float64}


def _engine(S=2, N=3, q="f64", shared=False, T=1, R=0, **cfg):
    from p2pmicrogrid_amd.engine import DeviceCommunityBatch
    return DeviceCommunityBatch(S, N, R, T, q_dtype=q, shared_q=shared, **cfg)


def _own(eng, first=0, count=None):
    """get_q in the tables' own dtype, [count, n_states, n_actions]"""
    q = eng.get_q(first, count, dtype=DT[eng.q_dtype])
    return q.reshape(q.shape[0], -1, q.shape[-1])


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(ref.bits(a), ref.bits(b))


def _ranges(n):
    """everything, the first table, the last, and a middle pair"""
    r = [(0, None), (0, 1), (n - 1, 1)]
    if n >= 3:
        r.append(((n - 2) // 2, 2))
    return r


def _check_export(eng, first=0, count=None, tag=""):
    q = _own(eng, first, count)
    got = eng.get_q_sparse(first, count)
    ref.assert_sparse_equal(got, q, eng.q_shape, tag=tag)
    n = eng.sparse_count(first, count)
    assert n.dtype == np.int64 and np.array_equal(n, np.diff(got["offsets"])), (tag, n)
    with np.errstate(over="ignore"):  # f64 max -> f32 inf, as the cast of get_q gives it
        ref.assert_sparse_equal(eng.get_q_sparse(first, count, dtype=OTHER[eng.q_dtype]), q, eng.q_shape,
                                dtype=OTHER[eng.q_dtype], tag=tag + " other dtype")
    return got


@pytest.mark.parametrize("q", ["f64", "f32"])
@pytest.mark.parametrize("shared,n_tables", [(False, 6), (True, 1), ("role", 3)])
@pytest.mark.parametrize("shape,na", [(SMALL, 3), (SMALL, 2), (ODD, 3)], ids=["120x3", "120x2", "81x3"])
def test_small_tables_every_mode_and_range(shape, na, shared, n_tables, q):
    eng = _engine(2, 3, q, shared, n_actions=na, **shape)
    assert eng.n_tables == n_tables and eng.q_shape[-1] == na
    fresh = _check_export(eng, tag="fresh")  # all zero: nothing stored
    assert fresh["rows"].size == 0 and fresh["values"].shape == (0, na) and not fresh["offsets"].any()
    t = ref.tables(n_tables, eng.n_states, na, q)
    eng.set_q(t)
    assert _same(_own(eng), t)
    for first, count in _ranges(n_tables):
        _check_export(eng, first, count, tag=f"{first}+{count}")
    # stored is a superset of visited: it differs by the rows of zeros with a -0.0 among them ...
    n, vis = eng.sparse_count(), eng.table_stats()["visited"]
    neg = (ref.stored(t) & ~(t != 0).any(axis=-1)).sum(axis=1)
    assert neg[0] >= 2 and np.array_equal(n - vis, neg)
    # ... and equals it on the same tables without them
    eng.set_q(ref.tables(n_tables, eng.n_states, na, q, neg_zero_rows=False))
    assert np.array_equal(eng.sparse_count(), eng.table_stats()["visited"]) and eng.sparse_count().sum() > 0


@pytest.mark.parametrize("q", ["f64", "f32"])
def test_full_size_tables_many_blocks_and_staging_runs(q):
    from p2pmicrogrid_amd import _lib
    eng = _engine(1, 3, q, **FULL)
    assert eng.n_states == 160000 and eng.n_states % 1024 != 0  # blocks of whole 1024-row tiles: a tail block
    t = ref.tables(3, eng.n_states, 3, q, seed=11, zero_table=False)
    eng.set_q(t)
    n = eng.sparse_count()
    assert n[2] == eng.n_states and (n[:2] > eng.n_states // 2).all() and (n[:2] < eng.n_states).all()
    if q == "f64":
        # 4 B of index and 3 x 8 B of values a row: the three tables do not fit one staging run, and the
        # full table alone does (a later change of the bound must keep both true, or change this test)
        assert int(n.sum()) * (4 + 3 * 8) > _lib.SPARSE_STAGE_BYTES >= int(n[2]) * (4 + 3 * 8)
        assert int(n[:2].sum()) * (4 + 3 * 8) <= _lib.SPARSE_STAGE_BYTES  # run 1: tables 0 and 1; run 2: table 2
    for first, count in _ranges(3):
        _check_export(eng, first, count, tag=f"{first}+{count}")
    # the import of more than one run
    sp = eng.get_q_sparse()
    eng.zero_q()
    eng.set_q_sparse(sp)
    assert _same(_own(eng), t)


@pytest.mark.parametrize("shape,q", [(SMALL, "f64"), (ODD, "f32")], ids=["120-f64", "81-f32"])
def test_import(shape, q, tmp_path):
    eng = _engine(2, 3, q, **shape)
    n, ns, dt = eng.n_tables, eng.n_states, DT[q]
    t = ref.tables(n, ns, 3, q, seed=17)
    eng.set_q(t)
    sp = eng.get_q_sparse()
    # zero, then import: the original, bit for bit (-0.0 rows included; an all-+0.0 row is simply absent)
    eng.zero_q()
    eng.set_q_sparse(sp)
    assert _same(_own(eng), t)
    # zero=True over non-zero tables: they become the form's tables
    base = np.random.RandomState(1).standard_normal((n, ns, 3)).astype(dt) + dt(9)
    eng.set_q(base)
    eng.set_q_sparse(sp, zero=True)
    assert _same(_own(eng), t)
    # zero=False over non-zero tables: exactly the listed rows change
    eng.set_q(base)
    eng.set_q_sparse(sp, zero=False)
    want = np.where(ref.stored(t)[..., None], t, base)
    assert _same(_own(eng), want) and not _same(want, t) and not _same(want, base)
    # a sub-range leaves the other tables untouched, with and without zeroing
    for zero in (True, False):
        eng.set_q(base)
        part = {"shape": sp["shape"], "offsets": sp["offsets"][2:5] - sp["offsets"][2],
                "rows": sp["rows"][sp["offsets"][2]:sp["offsets"][4]],
                "values": sp["values"][sp["offsets"][2]:sp["offsets"][4]]}
        eng.set_q_sparse(part, first=3, zero=zero)  # tables 2 and 3 of the form over tables 3 and 4
        want = base.copy()
        want[3:5] = t[2:4] if zero else np.where(ref.stored(t[2:4])[..., None], t[2:4], base[3:5])
        assert _same(_own(eng), want), zero
    # values of the other dtype are converted as set_q converts them
    eng.zero_q()
    with np.errstate(over="ignore"):
        other = {**sp, "values": sp["values"].astype(OTHER[q])}
    eng.set_q_sparse(other)
    want = np.zeros_like(t)
    want[ref.stored(t)] = other["values"].astype(dt)
    assert _same(_own(eng), want)
    # a form of another table shape
    with pytest.raises(ValueError):
        eng.set_q_sparse({**sp, "shape": np.asarray((*eng.q_shape[:-1], 2))})
    # the file format, into a second context
    eng.set_q(t)
    path = eng.save_tables(str(tmp_path / "tables"), first=1, count=4)
    assert path.endswith("tables.npz")
    with np.load(path, allow_pickle=False) as f:
        assert sorted(f.files) == ["offsets", "rows", "shape", "values"]
        assert f["offsets"].dtype == np.int64 and f["rows"].dtype == np.int32 and f["values"].dtype == dt
        assert tuple(f["shape"]) == eng.q_shape and f["offsets"].shape == (5,)
    two = _engine(2, 3, q, **shape)
    two.set_q(base)
    assert two.load_tables(path, first=2) == 4
    want = base.copy()
    want[2:6] = t[1:5]
    assert _same(_own(two), want)
    wrong = _engine(2, 3, q, **(ODD if shape is SMALL else SMALL))
    with pytest.raises(ValueError):
        wrong.load_tables(path)


def test_actor_bound_to_a_device_saves_and_loads(tmp_path):
    from p2pmicrogrid_amd.rl import QActor
    t = ref.tables(1, 120, 3, "f64", seed=4)[0].reshape(3, 4, 5, 2, 3)
    a = QActor(3, 4, 5, 2)
    a.set_qtable(t)
    a._device()  # binds to a private one-agent context
    path = str(tmp_path / "actor.npz")
    a.save_sparse(path)
    b = QActor(3, 4, 5, 2)  # unbound: the same file format either way
    b.load_sparse(path)
    assert _same(b.q_table, t)
    a.set_qtable(np.ones_like(t))
    a.load_sparse(path)
    assert a._engine is not None and _same(a.q_table, t)


@pytest.mark.parametrize("shape,q", [(SMALL, "f64"), (ODD, "f32"), (FULL, "f64")], ids=["120-f64", "81-f32", "160000-f64"])
def test_copy_q(shape, q):
    from p2pmicrogrid_amd import _lib
    eng = _engine(2, 3, q, **shape)
    t = ref.tables(6, eng.n_states, 3, q, seed=29)
    eng.set_q(t)
    eng.copy_q(0, 2, 3)  # table 0 (first and last row stored) over tables 2, 3, 4
    want = t.copy()
    want[2:5] = t[0]
    assert _same(_own(eng), want)
    eng.copy_q(5, 0, 5)  # the last table over all the others: five destinations, three copies
    want[0:5] = t[5]
    assert _same(_own(eng), want)
    eng.copy_q(1, 0, 1)
    assert _same(_own(eng), want)
    for bad in ((2, 0, 3), (0, 0, 1), (4, 2, 3), (6, 0, 2), (-1, 0, 2), (0, 4, 3), (0, -1, 2), (0, 1, -1)):
        with pytest.raises(_lib.P2PMGError, match="INVALID"):
            eng.copy_q(*bad)
    assert _same(_own(eng), want)
    assert eng.L.p2pmg_copy_q(eng._ctx, 0, 3, 0) == 0  # count == 0


def _arr(values, dtype):
    a = np.ascontiguousarray(values, dtype)
    return a, a.ctypes.data


def test_refusals():
    from p2pmicrogrid_amd import _lib
    eng = _engine(2, 3, "f64", **SMALL)  # 6 tables of 120 rows
    L, ctx, ns = eng.L, eng._ctx, eng.n_states
    t = ref.tables(6, ns, 3, "f64", seed=31)
    eng.set_q(t)
    vals = np.full((8, 3), 5.0)

    def set_sparse(n_rows, rows, first=0, zero=1, values=vals):
        n, pn = _arr(n_rows, np.int64)
        r, pr = _arr(rows, np.int32)
        return L.p2pmg_set_q_sparse(ctx, first, len(n), pn, pr, values.ctypes.data, _lib.Q_F64, zero)

    for zero in (1, 0):  # zero_first must not have zeroed anything either
        assert set_sparse([2, 3], [4, 9, 7, 3, 8], zero=zero) == 1      # unsorted in the second table
        assert b"ascending" in L.p2pmg_last_error(ctx)
        assert set_sparse([3], [4, 9, 9], zero=zero) == 1               # duplicated
        assert set_sparse([2], [-1, 3], zero=zero) == 1                 # negative
        assert set_sparse([2, 1], [0, 5, ns], zero=zero) == 1           # out of range
        assert set_sparse([1, ns + 1], [0], zero=zero) == 1             # n_rows above n_states
        assert set_sparse([-1], [0], zero=zero) == 1                    # n_rows negative
        assert set_sparse([1], [0], first=6, zero=zero) == 1            # past the last table
        assert set_sparse([1, 1], [0, 0], first=5, zero=zero) == 1
        assert _same(_own(eng), t), zero
    n1, p1 = _arr([1], np.int64)
    r1, q1 = _arr([3], np.int32)
    assert L.p2pmg_set_q_sparse(ctx, 0, 1, None, q1, vals.ctypes.data, 0, 1) == 1      # null n_rows
    assert L.p2pmg_set_q_sparse(ctx, 0, 1, p1, None, vals.ctypes.data, 0, 1) == 1      # null rows
    assert L.p2pmg_set_q_sparse(ctx, 0, 1, p1, q1, None, 0, 1) == 1                    # null values
    assert L.p2pmg_set_q_sparse(ctx, 0, 1, p1, q1, vals.ctypes.data, 7, 1) == 1        # no dtype
    assert _same(_own(eng), t)
    # a sorted form with the same index in two tables is fine, and the last index may be n_states - 1
    assert set_sparse([2, 1], [4, ns - 1, 4], first=1, zero=0) == 0
    want = t.copy()
    want[1, [4, ns - 1]] = 5.0
    want[2, 4] = 5.0
    assert _same(_own(eng), want)
    eng.set_q(t)

    # capacity one short: n_rows filled, the buffers untouched; then exactly enough
    n_rows, rows, values = ref.sparse(t)
    total = int(n_rows.sum())
    got_n = np.full(6, -1, np.int64)
    got_r = np.full(total, -7, np.int32)
    got_v = np.full((total, 3), 123.0)
    call = lambda cap: L.p2pmg_get_q_sparse(ctx, 0, 6, cap, got_n.ctypes.data, got_r.ctypes.data,  # noqa: E731
                                            got_v.ctypes.data, _lib.Q_F64)
    assert call(total - 1) == 1 and b"capacity" in L.p2pmg_last_error(ctx)
    assert np.array_equal(got_n, n_rows) and (got_r == -7).all() and (got_v == 123.0).all()
    assert call(-1) == 1 and (got_r == -7).all()
    assert call(total) == 0
    assert np.array_equal(got_r, rows) and _same(got_v, values)
    assert L.p2pmg_get_q_sparse(ctx, 0, 6, total, None, got_r.ctypes.data, got_v.ctypes.data, 0) == 1
    assert L.p2pmg_get_q_sparse(ctx, 0, 6, total, got_n.ctypes.data, None, got_v.ctypes.data, 0) == 1
    assert L.p2pmg_get_q_sparse(ctx, 0, 6, total, got_n.ctypes.data, got_r.ctypes.data, None, 0) == 1
    assert L.p2pmg_get_q_sparse(ctx, 0, 6, total, got_n.ctypes.data, got_r.ctypes.data, got_v.ctypes.data, 2) == 1
    assert L.p2pmg_sparse_count(ctx, 0, 6, None) == 1
    for bad in ((5, 2), (-1, 1), (0, 7), (0, -1)):
        with pytest.raises(_lib.P2PMGError, match="INVALID"):
            eng.sparse_count(*bad)
        with pytest.raises(_lib.P2PMGError, match="INVALID"):
            eng.get_q_sparse(*bad)
    # count == 0: OK, nothing looked at (null pointers)
    assert L.p2pmg_sparse_count(ctx, 6, 0, None) == 0
    assert L.p2pmg_get_q_sparse(ctx, 3, 0, 0, None, None, None, 0) == 0
    assert L.p2pmg_set_q_sparse(ctx, 6, 0, None, None, None, 0, 1) == 0
    empty = eng.get_q_sparse(2, 0)
    assert empty["offsets"].tolist() == [0] and empty["rows"].shape == (0,) and empty["values"].shape == (0, 3)
    assert _same(_own(eng), t)
    # a DQN context has no Q-table
    dqn = _engine(1, 1, "f32", learner=_lib.LEARNER_DQN)
    none = {"shape": np.asarray(dqn.q_shape), "offsets": np.zeros(2, np.int64), "rows": np.zeros(0, np.int32),
            "values": np.zeros((0, 3))}
    for call in (dqn.sparse_count, dqn.get_q_sparse, lambda: dqn.copy_q(0, 0, 1), lambda: dqn.set_q_sparse(none)):
        with pytest.raises(_lib.P2PMGError, match="STATE.*no Q-table"):
            call()
    assert dqn.L.p2pmg_get_q_sparse(dqn._ctx, 0, 1, 0, got_n.ctypes.data, None, None, 0) == 4


def test_shared_table_export_ignores_the_pending_delta_and_the_snapshot():
    eng = _engine(2, 3, "f64", True, **SMALL)
    t = ref.tables(1, eng.n_states, 3, "f64", seed=2)
    eng.set_q(t)
    eng.policy_mark()
    d = np.zeros(eng.q_shape, np.int64)
    d[..., 2] = 1 << 50
    eng.set_q_delta(d)
    sp = _check_export(eng, tag="pending")
    assert np.array_equal(np.diff(sp["offsets"]), ref.sparse(t)[0])  # the delta is not applied
    eng.set_q_sparse(sp)
    assert np.array_equal(eng.get_q_delta(), d)  # nor dropped by the zeroing import
    assert not eng.policy_changes(remark=False)["changed"].any()
    eng.apply_q_delta()
    assert eng.sparse_count()[0] == eng.n_states


def test_resume_from_a_sparse_export_is_exact():
    """Two Philox training episodes at S = 2, N = 2, R = 1, T = 96 (the fast kernel), exported; a fresh
    context with the same inputs imports the export, and episode 2 from the same temperatures leaves the
    same tables in both, bit for bit.  A 192-step history writes at most 2 x 96 x (R + 1) rows per agent."""
    from p2pmicrogrid_amd.dataset import scenario_batch
    S, N, T = 2, 2, 96
    inp = scenario_batch(S, N, T, seed=61)
    alpha = np.array([[1e-5, 2e-5], [3e-5, 1e-5]])
    gamma = np.array([[0.9, 0.8], [0.95, 0.9]])

    def context():
        eng = _engine(S, N, "f64", T=T, R=1)
        eng.set_env(np.broadcast_to(inp.time, inp.t_out.shape), inp.t_out)
        eng.set_profiles(inp.load_w, inp.pv_w)
        eng.set_max_in(inp.max_in)
        eng.set_learning(alpha=alpha, gamma=gamma)
        return eng

    a = context()
    a.set_temperatures(inp.t_in0, inp.t_m0)
    for e in range(2):
        a.run_episode("train", "philox", episode=e, epsilon=0.5, reset_sigma=0.3)
    sp = _check_export(a, tag="trained")
    n_rows = np.diff(sp["offsets"])
    assert (n_rows > 0).all() and (n_rows < a.n_states / 10).all() and (n_rows <= 2 * T * 2).all(), n_rows
    t_in, t_m = a.get_temperatures()
    b = context()
    b.set_q_sparse(sp)
    before = _own(a)
    assert _same(_own(b), before)
    for eng in (a, b):
        eng.set_temperatures(t_in, t_m)
        eng.run_episode("train", "philox", episode=2, epsilon=0.5, reset_sigma=0.3)
    qa, qb = _own(a), _own(b)
    assert _same(qa, qb)
    assert not _same(qa, before)  # episode 2 did write
