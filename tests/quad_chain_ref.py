"""Host-side reference for four chained episodes per wave: access traces of a serial chain
taken from the oracle, the source of every wrap read (step T - 1's next-state row) under the K-group
schedule, and a NumPy model of the agents' tables under that schedule's lockstep order.

The model keeps, per agent and table row, the stores in lockstep order.  A load issued at lockstep step
x (the rows of step x + 1 are issued at step x, ahead of that step's TD store) sees
  * its own group's stores of steps <= x - 1, and the step-x store through the patch (as the kernel's Patch);
  * another group's stores of steps <= x - 4 for certain, of steps x - 3 .. x - 1 perhaps: the model
    evaluates both and counts a load whose two views differ as a mismatch, the wrap read aside;
and a group's first store into a row (key of step 0, temperature bin, p2p = 0) logs max3 of the row as it read it.
The wrap read takes the earliest follower's logged value (priority="earliest"); priority="next" is the
two-group rule (episode e + 1's log or the loaded row), which is wrong for four groups."""
import numpy as np

F32 = np.float32


def serial_traces(ob, run_one, n):
    """Run n chained episodes on the oracle batch ob (run_one(k) runs episode k and the T0 reset that
    follows it, returning the oracle's output dict) -> the trace dict of the serial chain, and a serial
    replay of the trace alone that must reproduce the oracle's table after every episode."""
    p = ob.params
    S, N, R, T = ob.S, ob.N, ob.R, ob.T
    A = S * N
    tr = dict(T=T, R=R, A=A, n=n, row=np.zeros((n, T, R + 1, A), np.int64), act=np.zeros((n, T, A), np.int64),
              nrow=np.zeros((n, T, A), np.int64), rew=np.zeros((n, T, A), F32), iT=np.zeros((n, T, A), np.int64),
              logs=np.zeros((n, T, A), bool))
    q = np.zeros((A, ob.n_states, 3), ob.q.dtype)
    qsa_s = np.zeros((n, T, A), q.dtype)
    qmax_s = np.zeros((n, T, A), q.dtype)
    new_s = np.zeros((n, T, A), q.dtype)
    rows_s = np.zeros((n, T, R + 1, A, 3), q.dtype)
    ar = np.arange(A)
    f64 = q.dtype == np.float64
    for e in range(n):
        out = run_one(e)
        idx = out["idx"].reshape(T, R + 1, A, 4)  # it, iT, ib, ip
        it, iT, ib, ip = (idx[..., k] for k in range(4))
        tr["row"][e] = ob._row(it, iT, ib, ip)
        tr["act"][e] = out["action"].reshape(T, R + 1, A)[:, R]
        tr["nrow"][e] = ob._row(np.roll(it[:, 0], -1, axis=0), iT[:, 0], np.roll(ib[:, 0], -1, axis=0), ip[:, 0])
        tr["rew"][e] = out["reward"].reshape(T, A)
        tr["iT"][e] = iT[:, 0]
        lo = it[:, 0] * 65536 + ib[:, 0]
        if e == 0:
            tr["lo"] = lo.T.copy()  # [A, T], the same for every episode
        # the steps whose store the undo log would record: step 0's key, the final round's p2p bin = the p2p = 0 bin
        tr["logs"][e] = (lo == lo[0]) & (ip[:, R] == ip[:, 0])
        for t in range(T):
            srow, a = tr["row"][e, t, R], tr["act"][e, t]
            for r in range(R + 1):
                rows_s[e, t, r] = q[ar, tr["row"][e, t, r]]
            qsa = q[ar, srow, a]
            qmax = q[ar, tr["nrow"][e, t]].max(axis=-1)
            rew = tr["rew"][e, t]
            if f64:
                new = qsa + p.alpha * ((rew.astype(np.float64) + p.gamma * qmax) - qsa)
            else:
                new = qsa + F32(p.alpha) * ((rew + F32(p.gamma) * qmax) - qsa)
            q[ar, srow, a] = new
            qsa_s[e, t], qmax_s[e, t], new_s[e, t] = qsa, qmax, new
        assert np.array_equal(q, ob.q), f"the trace replay left another table than the oracle after episode {e}"
    tr.update(qsa=qsa_s, qmax=qmax_s, new=new_s, rows=rows_s)
    return tr


def hazard_distance(lo):
    """chain_lag_kernel's D over keys lo [A, T] (lo-lo, lo-hi, hi-lo pairs; step T - 1's next-state read excepted)."""
    T = lo.shape[1]
    hi = np.roll(lo, -1, axis=1)
    ll = lo[:, :, None] == lo[:, None, :]
    lh = lo[:, :, None] == hi[:, None, :]
    hl = hi[:, :, None] == lo[:, None, :]
    hl[:, T - 1, :] = False
    u, v = np.nonzero((ll | lh | hl).any(axis=0))
    return int((u - v).max())


def wrap_sources(tr, K=4):
    """-> counts [K]: how many wrap reads (episode e with a successor, agent a) take their value from the
    loaded row (index 0) or from the log of episode e + j (index j), by the earliest-follower rule."""
    n, T, A = tr["n"], tr["T"], tr["A"]
    counts = np.zeros(K, np.int64)
    for e in range(n - 1):
        b = tr["iT"][e, T - 1]  # the bin of the wrap row, per agent
        src = np.zeros(A, np.int64)
        for j in range(K - 1, 0, -1):
            if e + j < n:
                logged = (tr["logs"][e + j] & (tr["iT"][e + j] == b[None, :])).any(axis=0)
                src = np.where(logged, j, src)
        counts += np.bincount(src, minlength=K)
    return counts


def lockstep_mismatches(tr, K=4, priority="earliest"):
    """Replay the trace under the K-group lockstep schedule -> the number of values fed to an action choice
    or a TD update that differ from the serial chain's (0: the schedule computes what the serial chain does)."""
    n, T, R, A = tr["n"], tr["T"], tr["R"], tr["A"]
    L = T // K
    assert T % K == 0
    bad = 0
    for a in range(A):
        stores = {}  # row -> [(step, group, action, value)] in lockstep order
        key_rows = tr["logs"]
        masks = [set() for _ in range(K)]
        logs = [dict() for _ in range(K)]

        def view(row, x, g, lag):
            v = np.zeros(3, tr["new"].dtype)
            for (s, gs, act, val) in stores.get(row, ()):
                if (gs == g and s <= x) or (gs != g and s <= x - lag):  # own: s == x is the patch
                    v[act] = val
            return v

        for ph in range(n + K - 1):
            for g in range(K):
                if g == ph % K:  # this group's prologue: its log starts empty
                    masks[g], logs[g] = set(), dict()
            for t in range(L):
                x = ph * L + t  # this lockstep step; its rows were issued at x - 1
                live = []
                for g in range(K):
                    e = ph - ((ph - g) % K)
                    if 0 <= e < n:
                        live.append((g, e, (ph - e) * L + t))
                todo = []
                for g, e, u in live:
                    rowv = None
                    for r in range(R + 1):
                        row = tr["row"][e, u, r, a]
                        sure, maybe = view(row, x - 1, g, 4), view(row, x - 1, g, 1)
                        bad += int(not (np.array_equal(sure, maybe) and np.array_equal(sure, tr["rows"][e, u, r, a])))
                        rowv = sure
                    nrow = tr["nrow"][e, u, a]
                    qm = [view(nrow, x - 1, g, lag).max() for lag in (4, 1)]
                    if u == T - 1 and e + 1 < n:  # the wrap read: the followers' logs first
                        b = tr["iT"][e, u, a]
                        for j in range(1, K if priority == "earliest" else 2):
                            gj = (g + j) % K
                            if e + j < n and b in masks[gj]:
                                qm = [logs[gj][b]] * 2
                                break
                    bad += int(not (qm[0] == qm[1] == tr["qmax"][e, u, a]))
                    todo.append((g, e, u, rowv))
                for g, e, u, rowv in todo:  # every lane's log write and TD store follow every lane's reads
                    b = tr["iT"][e, u, a]
                    if key_rows[e, u, a] and b not in masks[g]:
                        masks[g].add(b)
                        logs[g][b] = rowv.max()
                    stores.setdefault(tr["row"][e, u, R, a], []).append((x, g, tr["act"][e, u, a], tr["new"][e, u, a]))
    return bad
