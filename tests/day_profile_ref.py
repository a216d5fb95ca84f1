"""The day profile of an episode's [T, S, N] records, in NumPy: the records reduced over scenarios.

The definition: a sample is a pair (s, t) with s in the scenario range, group[s] = g >= 0,
t in the step range and t % period = p; it adds one fixed-point term per field to row [g][p][i] of each agent
i.  fix(x, k) = rint(f64(x) * 2^k) as int64 (round to nearest even), the sums are int64, the extrema f32 with
zeros as +0.0, and the community's G_t is the oracle's seq_sum over the agents.  Every result is an integer
or an extremum, so no result depends on any order or split: parts are compared with ``np.array_equal``."""
import numpy as np

from oracle.restatement import seq_sum

F32, F64, I64 = np.float32, np.float64, np.int64
SUM_FIELDS = ("samples", "cost", "reward", "grid_import", "grid_export", "p2p_import", "p2p_export", "hp", "load", "pv",
              "t_in", "discomfort_deg", "discomfort_steps", "action1", "action2", "importing")
EXTREMA_FIELDS = ("t_in_min", "t_in_max", "grid_min", "grid_max", "p2p_min", "p2p_max", "cost_min", "cost_max")
COM_SUM_FIELDS = ("samples", "grid_import", "grid_export", "importing")
COM_EXTREMA_FIELDS = ("grid_min", "grid_max")
SHIFT_W, SHIFT_DEG, SHIFT_MONEY = 16, 24, 28
ZERO = F32(0)


def fix(x, k):
    return np.rint(np.asarray(x, F32).astype(F64) * 2.0 ** k).astype(I64)


def _pos(x):
    return np.where(x > ZERO, x, ZERO).astype(F32)


def _neg(x):
    return np.where(x < ZERO, -x, ZERO).astype(F32)


def sample_terms(out, hp_levels, load_w, pv_w, lower, upper, reward=True):
    """(terms [T, S, N, 16] i64, values [T, S, N, 4] f32 {T_in, grid, p2p, cost}, G [T, S] f32) per sample.
    out: cost, reward, grid, p2p, t_in [T, S, N] and action [T, R+1, S, N]; hp_levels [S, N, 3]; load_w, pv_w
    [S, N, T]; lower, upper: [S, N] (or scalar) f32 comfort bounds."""
    cost, grid, p2p, t_in = (np.asarray(out[k], F32) for k in ("cost", "grid", "p2p", "t_in"))
    T, S, N = cost.shape
    rew = np.asarray(out["reward"], F32) if reward else np.zeros((T, S, N), F32)
    act = np.asarray(out["action"])[:, -1].astype(I64)  # the final round's
    lv = np.concatenate([np.asarray(hp_levels, F32).reshape(S, N, 3), np.zeros((S, N, 1), F32)], axis=-1)
    hp = np.take_along_axis(np.broadcast_to(lv, (T, S, N, 4)), act[..., None], axis=-1)[..., 0]
    load = np.moveaxis(np.asarray(load_w, F32).reshape(S, N, T), -1, 0)
    pv = np.moveaxis(np.asarray(pv_w, F32).reshape(S, N, T), -1, 0)
    lower = np.broadcast_to(np.asarray(lower, F32), (S, N))
    upper = np.broadcast_to(np.asarray(upper, F32), (S, N))
    lo, hi = _pos((lower - t_in).astype(F32)), _pos((t_in - upper).astype(F32))
    d = np.where(lo > hi, lo, hi).astype(F32)
    terms = np.stack([np.ones((T, S, N), I64), fix(cost, SHIFT_MONEY), fix(rew, SHIFT_MONEY),
                      fix(_pos(grid), SHIFT_W), fix(_neg(grid), SHIFT_W), fix(_pos(p2p), SHIFT_W), fix(_neg(p2p), SHIFT_W),
                      fix(hp, SHIFT_W), fix(load, SHIFT_W), fix(pv, SHIFT_W), fix(t_in, SHIFT_DEG), fix(d, SHIFT_DEG),
                      (d > ZERO).astype(I64), (act == 1).astype(I64), (act == 2).astype(I64), (grid > ZERO).astype(I64)],
                     axis=-1)
    values = np.stack([t_in, grid, p2p, cost], axis=-1).astype(F32)
    return terms, values, seq_sum(grid, axis=-1)


def _ranges(T, S, period, steps, scenarios, groups, n_groups):
    """The arguments' conventions: period None or 0 = T (no folding); steps, scenarios = (first, stop), half
    open, None = all (a call that takes (first, count) passes count = stop - first); groups None = every
    scenario in group 0; n_groups None = max(label) + 1, 0 = 1."""
    P = T if not period else int(period)
    t0, t1 = (0, T) if steps is None else steps
    s0, s1 = (0, S) if scenarios is None else scenarios
    if not (1 <= P <= T and 0 <= t0 <= t1 <= T and 0 <= s0 <= s1 <= S):
        raise ValueError("period outside [0, T] or a range outside [0, T] / [0, S]")
    lab = np.zeros(S, I64) if groups is None else np.asarray(groups, I64)
    G = int(max(lab.max(), 0)) + 1 if n_groups is None else max(int(n_groups), 1)
    if lab.shape != (S,) or lab.min() < -1 or lab.max() >= G:
        raise ValueError("one label per scenario, each in [-1, n_groups)")
    return P, np.arange(t0, t1), np.arange(s0, s1), lab, G


def profile(out, hp_levels, load_w, pv_w, lower, upper, reward=True, period=None, steps=None, scenarios=None,
            groups=None, n_groups=None):
    """(sums [G, P, N, 16] i64, extrema [G, P, N, 8] f32, com_sums [G, P, 4] i64, com_extrema [G, P, 2] f32).
    steps, scenarios: (first, stop) or None; groups: [S] labels (-1: left out) or None."""
    terms, values, G_t = sample_terms(out, hp_levels, load_w, pv_w, lower, upper, reward)
    T, S, N = values.shape[:3]
    P, ts, ss, lab, G = _ranges(T, S, period, steps, scenarios, groups, n_groups)
    sums = np.zeros((G, P, N, 16), I64)
    ext = np.empty((G, P, N, 8), F32)
    ext[..., 0::2], ext[..., 1::2] = np.inf, -np.inf
    csums = np.zeros((G, P, 4), I64)
    cext = np.empty((G, P, 2), F32)
    cext[..., 0], cext[..., 1] = np.inf, -np.inf
    for g in range(G):
        sg = ss[lab[ss] == g]
        for p in range(P):
            tp = ts[ts % P == p]
            if sg.size == 0 or tp.size == 0:
                continue
            ix = np.ix_(tp, sg)
            sums[g, p] = terms[ix].sum(axis=(0, 1), dtype=I64)
            v = values[ix]
            ext[g, p, :, 0::2] = v.min(axis=(0, 1)) + ZERO  # -0.0 + 0.0 = +0.0
            ext[g, p, :, 1::2] = v.max(axis=(0, 1)) + ZERO
            gt = G_t[ix]
            csums[g, p] = [gt.size, fix(_pos(gt), SHIFT_W).sum(dtype=I64), fix(_neg(gt), SHIFT_W).sum(dtype=I64),
                           int((gt > ZERO).sum())]
            cext[g, p] = [gt.min() + ZERO, gt.max() + ZERO]
    return sums, ext, csums, cext


def _fix_scalar(x, k):
    """fix of one f32 with Python numbers: float(x) * 2^k is exact in a double, round() goes to nearest even."""
    return round(float(F32(x)) * 2.0 ** k)


def profile_loops(out, hp_levels, load_w, pv_w, lower, upper, reward=True, period=None, steps=None, scenarios=None,
                  groups=None, n_groups=None):
    """The same arrays by a plain loop over (t, s, i): every term formed here from the records with scalar f32
    arithmetic and Python integers, sharing nothing with ``profile`` but the argument conventions."""
    T, S, N = np.shape(out["cost"])
    P, ts, ss, lab, G = _ranges(T, S, period, steps, scenarios, groups, n_groups)
    levels = np.asarray(hp_levels, F32).reshape(S, N, 3)
    load_w, pv_w = np.asarray(load_w, F32).reshape(S, N, T), np.asarray(pv_w, F32).reshape(S, N, T)
    lower = np.broadcast_to(np.asarray(lower, F32), (S, N))
    upper = np.broadcast_to(np.asarray(upper, F32), (S, N))
    sums = [[[[0] * 16 for _ in range(N)] for _ in range(P)] for _ in range(G)]
    ext = np.empty((G, P, N, 8), F32)
    ext[..., 0::2], ext[..., 1::2] = np.inf, -np.inf
    csums = [[[0] * 4 for _ in range(P)] for _ in range(G)]
    cext = np.empty((G, P, 2), F32)
    cext[..., 0], cext[..., 1] = np.inf, -np.inf
    for t in ts:
        p = int(t) % P
        for s in ss:
            g = int(lab[s])
            if g < 0:
                continue
            gt = F32(0)
            for i in range(N):
                cost, grid, p2p, tin = (F32(out[k][t][s][i]) for k in ("cost", "grid", "p2p", "t_in"))
                rew = F32(out["reward"][t][s][i]) if reward else ZERO
                act = int(out["action"][t][-1][s][i])
                hp = levels[s, i, act] if act < 3 else ZERO
                lo, hi = F32(lower[s, i] - tin), F32(tin - upper[s, i])
                lo, hi = (lo if lo > 0 else ZERO), (hi if hi > 0 else ZERO)
                d = lo if lo > hi else hi
                term = [1, _fix_scalar(cost, 28), _fix_scalar(rew, 28),
                        _fix_scalar(grid, 16) if grid > 0 else 0, _fix_scalar(-grid, 16) if grid < 0 else 0,
                        _fix_scalar(p2p, 16) if p2p > 0 else 0, _fix_scalar(-p2p, 16) if p2p < 0 else 0,
                        _fix_scalar(hp, 16), _fix_scalar(load_w[s, i, t], 16), _fix_scalar(pv_w[s, i, t], 16),
                        _fix_scalar(tin, 24), _fix_scalar(d, 24), int(d > 0), int(act == 1), int(act == 2), int(grid > 0)]
                row = sums[g][p][i]
                for f in range(16):
                    row[f] += term[f]
                for f, x in enumerate((tin, grid, p2p, cost)):
                    x = x + ZERO  # -0.0 + 0.0 = +0.0
                    ext[g, p, i, 2 * f] = min(ext[g, p, i, 2 * f], x)
                    ext[g, p, i, 2 * f + 1] = max(ext[g, p, i, 2 * f + 1], x)
                gt = F32(gt + grid)
            c = csums[g][p]
            c[0] += 1
            c[1] += _fix_scalar(gt, 16) if gt > 0 else 0
            c[2] += _fix_scalar(-gt, 16) if gt < 0 else 0
            c[3] += int(gt > 0)
            cext[g, p, 0] = min(cext[g, p, 0], gt + ZERO)
            cext[g, p, 1] = max(cext[g, p, 1], gt + ZERO)
    return np.array(sums, I64).reshape(G, P, N, 16), ext, np.array(csums, I64).reshape(G, P, 4), cext
