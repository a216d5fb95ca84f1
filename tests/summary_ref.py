"""Expected values of p2pmg_episode_summary, in NumPy, from an oracle episode's records.

The definition (include/p2pmg.h): per agent every field is accumulated in f64 sequentially over
t = 0..T-1 from +0.0, each term formed in f32 and then widened; per scenario fields 0-11 are the
sequential f64 sum over i = 0..N-1 of the agents' values, 12 / 13 the min / max over the agents, and
14 / 15 the community's peaks of G_t, the sequential f32 sum over i of grid[t, s, i].  The loops
below run over t and i in exactly that order (vectorised over the independent agents / scenarios
only), so the device's arrays are compared with ``np.array_equal``.
"""
import numpy as np

F32, F64 = np.float32, np.float64
FIELDS = ("cost", "reward", "grid_import", "grid_export", "p2p_import", "p2p_export", "hp", "load", "pv",
          "self_consumption", "discomfort_deg", "discomfort_steps", "t_in_min", "t_in_max", "peak_import",
          "peak_export")
ZERO = F32(0)


def _pos(x):
    return np.where(x > ZERO, x, ZERO).astype(F32)


def _neg(x):
    return np.where(x < ZERO, -x, ZERO).astype(F32)


def agent_summary(cost, reward, grid, p2p, t_in, action, hp_levels, load_w, pv_w, lower, upper):
    """[S, N, 16] f64.  cost, grid, p2p, t_in: [T, S, N] f32; reward: the same or None (not recorded);
    action: [T, R+1, S, N] integer; hp_levels: [S, N, 3] f32; load_w, pv_w: [S, N, T] f32; lower,
    upper: [S, N] f32 comfort bounds."""
    cost, grid, p2p, t_in = (np.asarray(x, F32) for x in (cost, grid, p2p, t_in))
    T, S, N = cost.shape
    lv = np.concatenate([np.asarray(hp_levels, F32).reshape(S, N, 3), np.zeros((S, N, 1), F32)], axis=-1)
    load_w, pv_w = np.asarray(load_w, F32).reshape(S, N, T), np.asarray(pv_w, F32).reshape(S, N, T)
    lower = np.broadcast_to(np.asarray(lower, F32), (S, N))
    upper = np.broadcast_to(np.asarray(upper, F32), (S, N))
    out = np.zeros((S, N, 16), F64)
    t_min, t_max = np.full((S, N), np.inf, F32), np.full((S, N), -np.inf, F32)
    pk_in, pk_out = np.zeros((S, N), F32), np.zeros((S, N), F32)
    for t in range(T):
        g, pp, ti, pv = grid[t], p2p[t], t_in[t], pv_w[:, :, t]
        gi, ge = _pos(g), _neg(g)
        act = np.asarray(action[t][-1]).astype(np.int64)
        hp = np.take_along_axis(lv, act[..., None], axis=-1)[..., 0]
        power = (g + pp).astype(F32)
        sc = np.where(power < ZERO, (pv + power).astype(F32), pv).astype(F32)
        lo, hi = _pos((lower - ti).astype(F32)), _pos((ti - upper).astype(F32))
        d = np.where(lo > hi, lo, hi).astype(F32)
        rew = np.zeros((S, N), F32) if reward is None else np.asarray(reward[t], F32)
        terms = (cost[t], rew, gi, ge, _pos(pp), _neg(pp), hp, load_w[:, :, t], pv, sc, d)
        for k, x in enumerate(terms):
            out[..., k] = out[..., k] + x.astype(F64)
        out[..., 11] = out[..., 11] + np.where(d > ZERO, 1.0, 0.0)
        t_min = np.where(ti < t_min, ti, t_min)
        t_max = np.where(ti > t_max, ti, t_max)
        pk_in = np.where(gi > pk_in, gi, pk_in)
        pk_out = np.where(ge > pk_out, ge, pk_out)
    for k, x in ((12, t_min), (13, t_max), (14, pk_in), (15, pk_out)):
        out[..., k] = x.astype(F64)
    return out


def scenario_summary(agent, grid):
    """[S, 16] f64 from agent_summary's array and grid [T, S, N] f32."""
    grid = np.asarray(grid, F32)
    T, S, N = grid.shape
    out = np.zeros((S, 16), F64)
    out[:, 12], out[:, 13] = np.inf, -np.inf
    for i in range(N):
        out[:, :12] = out[:, :12] + agent[:, i, :12]
        out[:, 12] = np.where(agent[:, i, 12] < out[:, 12], agent[:, i, 12], out[:, 12])
        out[:, 13] = np.where(agent[:, i, 13] > out[:, 13], agent[:, i, 13], out[:, 13])
    pk_in, pk_out = np.zeros(S, F32), np.zeros(S, F32)
    for t in range(T):
        G = np.zeros(S, F32)
        for i in range(N):
            G = (G + grid[t, :, i]).astype(F32)
        gi, ge = _pos(G), _neg(G)
        pk_in = np.where(gi > pk_in, gi, pk_in)
        pk_out = np.where(ge > pk_out, ge, pk_out)
    out[:, 14], out[:, 15] = pk_in.astype(F64), pk_out.astype(F64)
    return out


def summary(out, hp_levels, load_w, pv_w, lower, upper, reward=True):
    """(agent [S, N, 16], scenario [S, 16]) from an OracleBatch.run_episode output (or any dict with
    cost, reward, grid, p2p, t_in [T, S, N] and action [T, R+1, S, N])."""
    ag = agent_summary(out["cost"], out["reward"] if reward else None, out["grid"], out["p2p"], out["t_in"],
                       out["action"], hp_levels, load_w, pv_w, lower, upper)
    return ag, scenario_summary(ag, out["grid"])
