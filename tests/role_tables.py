"""Expected values for per-role tables (``shared_q="role"``), from the per-agent oracle.

oracle/restatement.py has no role mode, so both tests of it (CPU and GPU) derive it here:

* frozen-table trick: a per-agent OracleBatch with alpha = 0 never changes its tables
  (qsa + 0 * x == qsa for finite x), so with agent (s, i)'s table set to role table i its records are
  the role-mode trajectory, in TRAIN mode too;
* delta helper: each agent-step's next-state row is rebuilt with the oracle's own state_index / _row
  (time at t + 1, the same temperature bin, the next balance, the p2p bin of 0 / max_in), and
  rint(alpha * ((r + gamma * max Q_i[ns]) - Q_i[s, a]) * 2^40) is summed per role with np.add.at.
"""
import dataclasses

import numpy as np

from oracle.restatement import DELTA_SCALE, OracleBatch, OracleParams, state_index

F32 = np.float32
N_STATES = 20 ** 4


def random_tables(N, q_dtype="f64", seed=5):
    """[N, n_states, 3] role tables with a non-trivial argmax."""
    q = np.random.RandomState(seed).standard_normal((N, N_STATES, 3))
    return q if q_dtype == "f64" else q.astype(F32)


def set_role_tables(ob, tables):
    """Agent (s, i) of the per-agent oracle reads a copy of role table i."""
    ob.q[:] = np.tile(np.asarray(tables).reshape(ob.N, ob.n_states, -1), (ob.S, 1, 1))


def frozen_oracle(inp, N, R, tables, q_dtype="f64", params=None, **kw):
    S = inp.load_w.shape[0]
    params = dataclasses.replace(params or OracleParams(), alpha=0.0)
    ob = OracleBatch(S=S, N=N, R=R, load_w=inp.load_w, pv_w=inp.pv_w, max_in=inp.max_in, env_time=inp.time[None],
                     env_tout=inp.t_out, q_dtype=q_dtype, params=params, **kw)
    set_role_tables(ob, tables)
    ob.t_in, ob.t_m = inp.t_in0.copy(), inp.t_m0.copy()
    return ob


def role_deltas(ob, out, tables, alpha=1e-5, gamma=0.9):
    """[N, n_states, 3] int64: the fixed-point TD deltas of one training episode whose records are
    ``out`` (run on tables frozen at ``tables``), summed per role."""
    p = ob.params
    S, N, R, T = ob.S, ob.N, ob.R, ob.T
    Q = np.asarray(tables).reshape(N, ob.n_states, -1)
    role = np.broadcast_to(np.arange(N), (S, N))
    delta = np.zeros(Q.shape, np.int64)
    for t in range(T):
        tn = (t + 1) % T
        idx = out["idx"][t, R]  # [S, N, 4] of the final round
        a = out["action"][t, R].astype(np.int64)
        time_n = ob._env(ob.env_time, tn)
        itn = state_index(np.broadcast_to(time_n[:, None], (S, N)), p.n_time, "time")
        ibn = state_index((ob.load_w[:, :, tn] - ob.pv_w[:, :, tn]) / ob.max_in, p.n_bal, "plain")
        ipn = state_index(np.zeros((S, N), F32) / ob.max_in, p.n_p2p, "plain")
        nrow = ob._row(itn, idx[..., 1], ibn, ipn)
        srow = ob._row(idx[..., 0], idx[..., 1], idx[..., 2], idx[..., 3])
        qmax = Q[role, nrow].max(axis=-1).astype(np.float64)
        qsa = Q[role, srow, a].astype(np.float64)
        d = alpha * ((out["reward"][t].astype(np.float64) + gamma * qmax) - qsa)
        np.add.at(delta, (role.ravel(), srow.ravel(), a.ravel()), np.rint(d * DELTA_SCALE).astype(np.int64).ravel())
    return delta


def applied(tables, delta):
    """Q + delta * 2^-40 in f64, cast to the tables' type, where delta != 0 (p2pmg_apply_q_delta)."""
    q = np.array(tables, copy=True)
    nz = delta != 0
    q[nz] = (q[nz].astype(np.float64) + delta[nz].astype(np.float64) * (1.0 / DELTA_SCALE)).astype(q.dtype)
    return q
