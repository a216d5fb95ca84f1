"""The sparse table form of include/p2pmg.h (p2pmg_sparse_count, p2pmg_get_q_sparse, p2pmg_set_q_sparse) in
plain NumPy, on an array q [tables, n_states, n_actions] (padding columns already dropped, as get_q()
returns them).  Written from the header alone; it shares no code with the package.

  stored row   one of the row's entries has a non-zero bit pattern: decided on the uint view, so that
               -0.0 is seen
  sparse form  n_rows [tables] i64, rows [total] i32 (ascending inside each table, table after table),
               values [total, n_actions]
"""
import numpy as np


def bits(q):
    q = np.ascontiguousarray(q)
    return q.view({8: np.uint64, 4: np.uint32}[q.dtype.itemsize])


def stored(q):
    """bool [tables, n_states]"""
    return (bits(q) != 0).any(axis=-1)


def sparse(q, dtype=None):
    """(n_rows, rows, values) of q [tables, n_states, n_actions]; storedness from q's own bits, values cast to
    dtype (None: q's) afterwards."""
    q = np.ascontiguousarray(q)
    s = stored(q)
    n_rows = s.sum(axis=1).astype(np.int64)
    rows = np.concatenate([np.flatnonzero(s[k]) for k in range(len(q))] + [np.zeros(0, np.int64)]).astype(np.int32)
    values = np.concatenate([q[k][s[k]] for k in range(len(q))] + [np.zeros((0, q.shape[-1]), q.dtype)])
    return n_rows, rows, values.astype(q.dtype if dtype is None else dtype)


def assert_sparse_equal(got, q, shape, dtype=None, tag=""):
    """got: DeviceCommunityBatch.get_q_sparse's dict; q: the same tables from get_q in the TABLE's dtype.
    Bit for bit, dtypes included."""
    n_rows, rows, values = sparse(q, dtype)
    assert set(got) == {"shape", "offsets", "rows", "values"}, (tag, sorted(got))
    assert got["shape"].dtype == np.int64 and tuple(got["shape"]) == tuple(shape), (tag, got["shape"])
    assert got["offsets"].dtype == np.int64 and got["offsets"].shape == (len(q) + 1,), (tag, got["offsets"])
    assert got["offsets"][0] == 0 and np.array_equal(np.diff(got["offsets"]), n_rows), (tag, got["offsets"], n_rows)
    assert got["rows"].dtype == np.int32 and np.array_equal(got["rows"], rows), (
        tag, np.flatnonzero(got["rows"] != rows)[:5] if got["rows"].shape == rows.shape else (got["rows"].shape, rows.shape))
    assert got["values"].dtype == values.dtype and got["values"].shape == values.shape, (tag, got["values"].dtype)
    assert np.array_equal(bits(got["values"]), bits(values)), (tag, np.argwhere(bits(got["values"]) != bits(values))[:5])


def tables(n_tables, n_states, na, q, seed=5, neg_zero_rows=True, zero_table=True):
    """[n_tables, n_states, na] in the context's element type ("f64" | "f32"): random normals with about a
    third of the rows zero; at scattered places rows of only -0.0 (stored, not visited), rows of mixed +0.0
    and -0.0, rows whose only non-zero entry is the last action, denormals and +-max; the first and the
    last row of table 0 stored (the last row a -0.0 row).  With two tables or more, table 1 is entirely
    zero (zero_table=False: it stays as drawn); with three or more, table 2 has every row stored.
    neg_zero_rows=False: the same tables with +0.0 wherever a row holds nothing but zeros, so that stored
    == visited."""
    dt = np.float64 if q == "f64" else np.float32
    fi = np.finfo(dt)
    rs = np.random.RandomState(seed)
    t = rs.standard_normal((n_tables, n_states, na)).astype(dt)
    t[rs.rand(n_tables, n_states) < 0.33] = 0
    last_only = np.zeros(na, dt)
    last_only[-1] = 0.5
    special = [np.full(na, -0.0, dt), np.array([0.0, -0.0, 0.0, -0.0][:na], dt), np.array([-0.0, 0.0, 0.0][:na], dt),
               last_only]
    for v in (fi.smallest_subnormal, -fi.smallest_subnormal, fi.tiny / 2, fi.max, -fi.max):
        for k in (0, na - 1):
            row = np.zeros(na, dt)
            row[k] = v
            special.append(row)
    special = np.stack(special)
    for a in range(n_tables):
        where = rs.permutation(n_states)[:len(special)]
        t[a, where] = special[:len(where)]
    t[0, 0] = special[3]
    t[0, -1] = special[0]
    if n_tables > 1 and zero_table:
        t[1] = 0
    if n_tables > 2:
        zero = ~stored(t[2:3])[0]
        t[2, zero] = rs.standard_normal((int(zero.sum()), na)).astype(dt) + dt(4)
        t[2, -1] = special[0]
    if not neg_zero_rows:
        t[~(t != 0).any(axis=-1)] = 0.0
    return t
