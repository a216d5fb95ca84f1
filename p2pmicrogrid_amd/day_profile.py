"""Day profiles: an episode's per-step records reduced over SCENARIOS, per time slot and agent position.

What an average day looks like across the scenarios of a launch (test days, weather draws, sweep arms): the
batched form of the reference's make_day_plot, make_baseline_day_plot, make_decisions_comparison_plot and
plot_grid_load (data_analysis.py: mean indoor temperature, heat-pump duty, cost and net grid load by time of
day).  One row per (group g, slot p = t % P, agent position i) and one per (g, p) for the community.

This module is the HOST form: ``from_records`` reduces records that are already in host memory, which is where
``CommunityMicrogrid.run()`` and ``run_days()`` put them anyway.  On a large batch (get_records of a
125,000 x 16 batch is 0.77 GB per record) use DeviceCommunityBatch.day_profile(), the device pass with this
definition (p2pmg_day_profile): it returns the same four arrays bit for bit.

The four arrays, bit for bit:
  sums        [G, P, N, 16] i64  per sample (s, t) of the row (SUM_FIELDS, fix shifts SUM_SHIFTS): 1; fix(cost, 28);
                                 fix(reward, 28) (0 when not recorded); fix at 16 of max(grid, 0), max(-grid, 0),
                                 max(p2p, 0), max(-p2p, 0), the heat-pump power of the final round's action, load,
                                 pv; fix(T_in, 24); fix(d, 24) and d > 0, d the distance outside the agent's comfort
                                 band (the summary's field 10); final-round action == 1, == 2; grid > 0
  extrema     [G, P, N, 8]  f32  min, max of T_in, grid, p2p, cost (zeros as +0.0); an empty row holds +inf, -inf
  com_sums    [G, P, 4]     i64  samples; fix at 16 of max(G_t, 0) and max(-G_t, 0); G_t > 0, with G_t the
                                 sequential f32 sum over i = 0..N-1 of grid[t, s, i] from +0.0 (plot_grid_load)
  com_extrema [G, P, 2]     f32  min, max of G_t
fix(x, k) = rint(f64(x) * 2^k) (to nearest even) as int64.  Every entry is an exact integer or an extremum, so
no entry depends on an order, and the arrays of disjoint scenario sets merge exactly (``merge``).  With at most
MAX_SAMPLES samples per row and magnitudes below 2^MAGNITUDE_BITS[k] (2^23 W, 2^15 degC, 2^11 money) no sum
reaches 2^63.  An f32 converts exactly from |x| >= 2^(23 - k) on (128 W, 0.5 degC, 2^-5 money), else to within
half a step: temperatures and most powers are exact, a single step's cost often is not.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np

F32, F64, I64 = np.float32, np.float64, np.int64
SHIFT_W, SHIFT_DEG, SHIFT_MONEY = 16, 24, 28
MAX_SAMPLES = 1 << 24
MAGNITUDE_BITS = {SHIFT_W: 23, SHIFT_DEG: 15, SHIFT_MONEY: 11}
SUM_FIELDS = ("samples", "cost", "reward", "grid_import", "grid_export", "p2p_import", "p2p_export", "hp", "load", "pv",
              "t_in", "discomfort_deg", "discomfort_steps", "action1", "action2", "importing")
SUM_SHIFTS = (0, 28, 28, 16, 16, 16, 16, 16, 16, 16, 24, 24, 0, 0, 0, 0)  # 0: a count
EXTREMA_FIELDS = ("t_in_min", "t_in_max", "grid_min", "grid_max", "p2p_min", "p2p_max", "cost_min", "cost_max")
COM_SUM_FIELDS = ("samples", "grid_import", "grid_export", "importing")
COM_EXTREMA_FIELDS = ("grid_min", "grid_max")
RECORDS = ("cost", "grid", "p2p", "t_in", "action")  # "reward" is optional (absent: column 2 is 0)
Arrays = Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]


def _fix(x, k):
    return np.rint(x.astype(F64) * 2.0 ** k).astype(I64)


def from_records(records: Dict[str, np.ndarray], hp_levels, load_w, pv_w, lower, upper, period: Optional[int] = None,
                 steps: Optional[Sequence[int]] = None, scenarios: Optional[Sequence[int]] = None, groups=None,
                 n_groups: Optional[int] = None) -> Arrays:
    """(sums, extrema, com_sums, com_extrema) of records in host memory, as get_records() returns them: cost,
    grid, p2p, t_in [T, S, N] f32, action [T, R+1, S, N], reward [T, S, N] if recorded.  hp_levels [S, N, 3] W,
    load_w, pv_w [S, N, T] W, lower, upper [S, N] (or scalar) comfort bounds, as the launch had them.
    period: P slots, slot(t) = t % P (None or 0: T, no folding; 96 folds a year of quarter hours into a day).
    steps, scenarios: (first, stop) half-open (None: all).  groups: [S] labels in [0, n_groups), -1 leaves a
    scenario out (None: one group); n_groups None: max(label) + 1, 0: 1."""
    missing = [k for k in RECORDS if k not in records]
    if missing:
        raise ValueError("day profile: the records lack " + ", ".join(missing))
    cost, grid, p2p, t_in = (np.asarray(records[k], F32) for k in ("cost", "grid", "p2p", "t_in"))
    T, S, N = cost.shape
    P = T if not period else int(period)
    t0, t1 = (0, T) if steps is None else (int(steps[0]), int(steps[1]))
    s0, s1 = (0, S) if scenarios is None else (int(scenarios[0]), int(scenarios[1]))
    if not (1 <= P <= T and 0 <= t0 <= t1 <= T and 0 <= s0 <= s1 <= S):
        raise ValueError("day profile: period outside [0, T], or a range outside [0, T] / [0, S]")
    lab = np.zeros(S, I64) if groups is None else np.asarray(groups).astype(I64).reshape(-1)
    G = int(max(lab.max(initial=0), 0)) + 1 if n_groups is None else max(int(n_groups), 1)
    if lab.shape != (S,) or (S and (lab.min() < -1 or lab.max() >= G)):
        raise ValueError("day profile: one label per scenario, each in [-1, n_groups)")
    ss = np.arange(s0, s1)
    ss = ss[lab[ss] >= 0]
    ts = np.arange(t0, t1)
    if ss.size and ts.size and np.bincount(lab[ss], minlength=G).max() * -(-ts.size // P) > MAX_SAMPLES:
        raise ValueError("day profile: more than 2^24 samples in one (group, slot, role): split by scenario range and "
                         "merge the parts")
    sel = np.ix_(ts, ss)
    cost, grid, p2p, t_in = cost[sel], grid[sel], p2p[sel], t_in[sel]  # [nt, ns, N]
    reward = np.asarray(records["reward"], F32)[sel] if "reward" in records else np.zeros_like(cost)
    act = np.asarray(records["action"])[:, -1][sel].astype(np.intp)  # the final round's
    lv = np.concatenate([np.asarray(hp_levels, F32).reshape(S, N, 3), np.zeros((S, N, 1), F32)], axis=-1)[ss]
    hp = np.take_along_axis(np.broadcast_to(lv, act.shape + (4,)), act[..., None], axis=-1)[..., 0]
    load = np.moveaxis(np.asarray(load_w, F32).reshape(S, N, T), -1, 0)[sel]
    pv = np.moveaxis(np.asarray(pv_w, F32).reshape(S, N, T), -1, 0)[sel]
    lower = np.broadcast_to(np.asarray(lower, F32), (S, N))[ss]
    upper = np.broadcast_to(np.asarray(upper, F32), (S, N))[ss]
    zero = F32(0)
    below, above = (lower - t_in).astype(F32), (t_in - upper).astype(F32)
    d = np.maximum(np.where(below > zero, below, zero), np.where(above > zero, above, zero)).astype(F32)
    ones = np.ones(cost.shape, I64)
    terms = np.stack([ones, _fix(cost, SHIFT_MONEY), _fix(reward, SHIFT_MONEY),
                      _fix(np.where(grid > zero, grid, zero), SHIFT_W), _fix(np.where(grid < zero, -grid, zero), SHIFT_W),
                      _fix(np.where(p2p > zero, p2p, zero), SHIFT_W), _fix(np.where(p2p < zero, -p2p, zero), SHIFT_W),
                      _fix(hp, SHIFT_W), _fix(load, SHIFT_W), _fix(pv, SHIFT_W), _fix(t_in, SHIFT_DEG), _fix(d, SHIFT_DEG),
                      ones * (d > zero), ones * (act == 1), ones * (act == 2), ones * (grid > zero)], axis=-1)
    values = np.stack([t_in, grid, p2p, cost], axis=-1) + zero  # -0.0 + 0.0 = +0.0
    g_t = np.zeros(cost.shape[:2], F32)
    for i in range(N):  # sequential over the agents, in f32
        g_t = (g_t + grid[..., i]).astype(F32)
    row = lab[ss][None, :] * P + (ts % P)[:, None]  # [nt, ns]: g P + p
    sums = np.zeros((G * P, N, 16), I64)
    mins = np.full((G * P, N, 4), np.inf, F32)
    maxs = np.full((G * P, N, 4), -np.inf, F32)
    np.add.at(sums, row, terms)
    np.minimum.at(mins, row, values)
    np.maximum.at(maxs, row, values)
    com = np.stack([np.ones(g_t.shape, I64), _fix(np.where(g_t > zero, g_t, zero), SHIFT_W),
                    _fix(np.where(g_t < zero, -g_t, zero), SHIFT_W), (g_t > zero).astype(I64)], axis=-1)
    com_sums = np.zeros((G * P, 4), I64)
    com_min, com_max = np.full(G * P, np.inf, F32), np.full(G * P, -np.inf, F32)
    np.add.at(com_sums, row, com)
    np.minimum.at(com_min, row, g_t + zero)
    np.maximum.at(com_max, row, g_t + zero)
    extrema = np.stack([mins, maxs], axis=-1).reshape(G, P, N, 8)  # min, max interleaved per value
    return (sums.reshape(G, P, N, 16), extrema, com_sums.reshape(G, P, 4),
            np.stack([com_min, com_max], axis=-1).reshape(G, P, 2))


def merge(parts: Sequence[Arrays]) -> Arrays:
    """The day profile of the union of disjoint scenario sets (scenario ranges of one launch, the shards of a
    batch) from their profiles of equal shapes: the integer arrays add, the extrema take the minimum of the
    even columns and the maximum of the odd ones.  Equal, bit for bit and in any order of the parts, to the
    profile computed over all the scenarios at once."""
    parts = list(parts)
    if not parts:
        raise ValueError("day profile merge: nothing to merge")
    sums = np.array(parts[0][0], I64, copy=True)
    ext = np.array(parts[0][1], F32, copy=True)
    csums = np.array(parts[0][2], I64, copy=True)
    cext = np.array(parts[0][3], F32, copy=True)
    for s, e, cs, ce in parts[1:]:
        if np.shape(s) != sums.shape or np.shape(e) != ext.shape or np.shape(cs) != csums.shape or np.shape(ce) != cext.shape:
            raise ValueError("day profile merge: the parts differ in shape (groups, period, agents)")
        sums += np.asarray(s, I64)
        csums += np.asarray(cs, I64)
        for acc, x in ((ext, np.asarray(e, F32)), (cext, np.asarray(ce, F32))):
            acc[..., 0::2] = np.minimum(acc[..., 0::2], x[..., 0::2])
            acc[..., 1::2] = np.maximum(acc[..., 1::2], x[..., 1::2])
    return sums, ext, csums, cext


def as_dict(sums, extrema, com_sums, com_extrema, energy_scale: float = 1.0) -> Dict[str, Dict[str, np.ndarray]]:
    """The four arrays as {"agent": {name: [G, P, N] f64}, "community": {name: [G, P] f64}}: "samples"; the means
    sum 2^-k / samples of cost, reward, grid_import, ..., t_in, discomfort_deg (NaN where samples = 0); the shares
    "discomfort", "action0", "action1", "action2", "importing"; "net_grid", "net_p2p" (import - export); and the
    extrema.  energy_scale multiplies the mean powers (time_slot / 60 * 1e-3 gives kWh per step), not the extrema."""
    def mean(total, n, shift, scale=1.0):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(n > 0, total.astype(F64) * (2.0 ** -shift * scale) / n, np.nan)
    n = sums[..., 0]
    f = {name: sums[..., j] for j, name in enumerate(SUM_FIELDS)}
    agent = {"samples": n.astype(F64)}
    for name, k in zip(SUM_FIELDS[1:12], SUM_SHIFTS[1:12]):
        agent[name] = mean(f[name], n, k, energy_scale if k == SHIFT_W else 1.0)
    agent["net_grid"] = mean(f["grid_import"] - f["grid_export"], n, SHIFT_W, energy_scale)
    agent["net_p2p"] = mean(f["p2p_import"] - f["p2p_export"], n, SHIFT_W, energy_scale)
    agent["discomfort"] = mean(f["discomfort_steps"], n, 0)
    agent["action0"] = mean(n - f["action1"] - f["action2"], n, 0)
    agent["action1"] = mean(f["action1"], n, 0)
    agent["action2"] = mean(f["action2"], n, 0)
    agent["importing"] = mean(f["importing"], n, 0)
    for j, name in enumerate(EXTREMA_FIELDS):
        agent[name] = extrema[..., j].astype(F64)
    cn = com_sums[..., 0]
    com = {"samples": cn.astype(F64),
           "grid_import": mean(com_sums[..., 1], cn, SHIFT_W, energy_scale),
           "grid_export": mean(com_sums[..., 2], cn, SHIFT_W, energy_scale),
           "net_grid": mean(com_sums[..., 1] - com_sums[..., 2], cn, SHIFT_W, energy_scale),
           "importing": mean(com_sums[..., 3], cn, 0),
           "grid_min": com_extrema[..., 0].astype(F64), "grid_max": com_extrema[..., 1].astype(F64)}
    return {"agent": agent, "community": com}
