"""Inputs and CPU-side predicates of the shared-table TD-delta tests (test_gpu_shared_delta.py,
test_cpu_shared_delta.py).  Nothing here touches the device at import: the builders are NumPy, the
predicates read the oracle's output only, and `engine_for` imports the package when it is called.

The shared-table path (p2pmg_tabular.h: lds_add_by_key / lds_hash_flush) rounds each agent-step's f64
TD delta to int64 fixed point (2^-40), adds it into a 2048-slot LDS hash per workgroup, flushes the
hash every 8 steps into one of 8 replicas and folds the replicas.  The builders here drive the parts
of it that scenario_batch inputs never reach:
  crowded_inputs     more distinct (state, action) keys per 8-step window than the hash has slots
  wide_delta_inputs  |delta| on both sides of 2^51 (sq16's two-instruction rounding and its fallback)
and the predicates prove from the oracle alone that they do."""
from __future__ import annotations

from dataclasses import dataclass
from fractions import Fraction
from typing import List, Optional

import numpy as np

from oracle.restatement import DELTA_SCALE, OracleBatch, OracleParams

F32 = np.float32
REC = ["reward", "cost", "grid", "p2p", "t_in", "action", "index"]
HASH_SLOTS = 2048       # kSqSlots (p2pmg_tabular.h)
FLUSH_STEPS = 8         # kSqFlushSteps
SQ16_WG_SCENARIOS = 32  # episode_sq16_kernel: 8 waves x 4 scenarios around one hash
BATTERY_J = 10 * 3.6e6


@dataclass
class CaseInputs:
    time: np.ndarray      # [S, T] f32 normalised slot of the day, per scenario
    t_out: np.ndarray     # [S, T] f32
    load_w: np.ndarray    # [S, N, T] f32
    pv_w: np.ndarray      # [S, N, T] f32
    max_in: np.ndarray    # [S, N] f32
    t_in0: np.ndarray     # [S, N] f32
    t_m0: np.ndarray      # [S, N] f32
    hp_levels: np.ndarray  # [S, N, 3] f32 heat-pump power per action
    capacity: np.ndarray  # [S, N] f64 battery capacity in J (used where a case runs with storage)
    prices: Optional[tuple] = None  # (buy, inj, p2p) [S, T] f32; None: the default price table of `time`
    alpha: Optional[float] = None   # the learner's alpha; None: the config's 1e-5

    @property
    def S(self):
        return self.load_w.shape[0]

    @property
    def N(self):
        return self.load_w.shape[1]

    @property
    def T(self):
        return self.load_w.shape[2]

    def rows(self, lo: int, hi: int) -> "CaseInputs":
        """Scenarios [lo, hi) as inputs of their own (a shard)."""
        pr = None if self.prices is None else tuple(x[lo:hi] for x in self.prices)
        return CaseInputs(self.time[lo:hi], self.t_out[lo:hi], self.load_w[lo:hi], self.pv_w[lo:hi], self.max_in[lo:hi],
                          self.t_in0[lo:hi], self.t_m0[lo:hi], self.hp_levels[lo:hi], self.capacity[lo:hi], pr, self.alpha)


# ----------------------------------------------------------------------------- A. crowded hash
def crowded_inputs(S: int, N: int, T: int, seed: int, mi_lo: float = 20.0, hp_max: float = 800.0,
                   cap_steps: float = 1.0) -> CaseInputs:
    """Ordinary inputs that spread the agents of a workgroup over as many (state, action) keys as the
    20^4 x 3 table allows: every bin of the key is close to uniform and independent between agents.
      time     a random slot per (scenario, step), never in the bin of the step before
      T_m0     uniform over [19.6, 22.4]: the comfort band [20, 22] (18 bins of 0.11 K) and a little
               either side; T_in0 within 0.3 K of it.  The indoor air follows the building mass within
               a few steps (heating.py:37-56), so a small heat pump (0 / 400 / 800 W) and an outdoor
               temperature of 10..18 degC keep T_in near where it started while its bin moves every step
      balance  load - PV uniform over [-max_in, max_in]: PV = 0 where it is positive, load = 0 where negative
      max_in   log-uniform over [20, 6000] W: the p2p feature is the peers' mean proposal over the
               agent's OWN max_in, so the small agents see it spread over the p2p bins
      battery  capacity = max_in x 900 s x U(0.2, 1): the usable 40 % of it absorbs a fraction of a
               step of the agent's own power, so the rule acts on most steps and seldom zeroes the net
               power (a zero net power in the comfort band is a zero reward and a zero delta)
    Epsilon = 1 in the first episode then draws the action uniformly."""
    rs = np.random.RandomState(seed)
    tbin = rs.randint(0, 20, (S, T))
    for t in range(1, T):  # a different time bin on every step
        same = tbin[:, t] == tbin[:, t - 1]
        tbin[same, t] = (tbin[same, t] + 1 + rs.randint(0, 19, same.sum())) % 20
    time = ((tbin + rs.uniform(0.1, 0.9, (S, T))) / 20.0).astype(F32)
    t_out = rs.uniform(10.0, 18.0, (S, T)).astype(F32)
    max_in = np.exp(rs.uniform(np.log(mi_lo), np.log(6000.0), (S, N))).astype(F32)
    net = rs.uniform(-1.0, 1.0, (S, N, T)) * max_in[..., None].astype(np.float64)
    load_w = np.where(net > 0, net, 0.0).astype(F32)
    pv_w = np.where(net < 0, -net, 0.0).astype(F32)
    t_m0 = rs.uniform(19.6, 22.4, (S, N)).astype(F32)
    t_in0 = (t_m0 + rs.uniform(-0.3, 0.3, (S, N))).astype(F32)
    lv = np.broadcast_to(np.array([0.0, 0.5 * hp_max, hp_max], F32), (S, N, 3)).copy()
    cap = max_in.astype(np.float64) * 900.0 * rs.uniform(0.2, cap_steps, (S, N))
    return CaseInputs(time, t_out, load_w, pv_w, max_in, t_in0, t_m0, lv, cap)


def final_keys(out) -> np.ndarray:
    """[T, S, N] int64: the oracle's delta key of every agent-step, the final round's (state, action)
    as the kernels form it: (((it * 20 + iT) * 20 + ib) * 20 + ip) * 4 + action."""
    idx = out["idx"][:, -1].astype(np.int64)  # [T, S, N, 4]
    row = ((idx[..., 0] * 20 + idx[..., 1]) * 20 + idx[..., 2]) * 20 + idx[..., 3]
    return row * 4 + out["action"][:, -1].astype(np.int64)


def first_episode_delta(out, alpha: float = OracleParams().alpha) -> np.ndarray:
    """[T, S, N] int64: the TD delta of every agent-step of a first episode on a zero table, where it
    is rint(alpha * r * 2^40) (the target and Q[s, a] are both zero), read from the reward record."""
    d = alpha * ((out["reward"].astype(np.float64) + 0.0) - 0.0)
    return np.rint(d * DELTA_SCALE).astype(np.int64)


def window_keys(out, first_scenario: int, n_scenarios: int, window: int = FLUSH_STEPS,
                alpha: float = OracleParams().alpha) -> List[int]:
    """Distinct delta keys per `window`-step window (the last one may be shorter) among scenarios
    [first_scenario, first_scenario + n_scenarios) of a first episode on a zero table, counting only
    agent-steps whose delta is non-zero: what one workgroup's hash is asked to hold between flushes."""
    keys = final_keys(out)[:, first_scenario:first_scenario + n_scenarios]
    nz = first_episode_delta(out, alpha)[:, first_scenario:first_scenario + n_scenarios] != 0
    T = keys.shape[0]
    return [int(np.unique(keys[t0:t0 + window][nz[t0:t0 + window]]).size) for t0 in range(0, T, window)]


def workgroup_window_keys(out, scen_per_wg: int, window: int = FLUSH_STEPS, role_keys: bool = False) -> List[List[int]]:
    """window_keys of every workgroup of scen_per_wg scenarios.  role_keys: per-role tables, whose keys
    carry the agent's position too."""
    S = out["reward"].shape[1]
    if role_keys:
        N = out["reward"].shape[2]
        out = dict(out)
        idx = out["idx"].astype(np.int64).copy()
        idx[..., 0] += 20 * np.arange(N)[None, None, None, :]  # any injective offset: only distinctness counts
        out["idx"] = idx
    return [window_keys(out, s0, min(scen_per_wg, S - s0), window) for s0 in range(0, S, scen_per_wg)]


# ----------------------------------------------------------------------------- B. wide deltas
WIDE_ALPHA = 0.05
WIDE_PEAK_STEPS = (0, 7)  # the second peak at a quarter of the first one's scale
# log2 of each scenario's price scale, off the peak steps and on step 0; four consecutive scenarios
# (64 agents) are one sq16 wave.  On step 0 wave 0 stays far below 2^51, wave 1 lies above it,
# waves 2 to 4 straddle it, and wave 5 (one scale for its four scenarios) lies wholly below it with
# its largest deltas just under it: negative values of a magnitude in [2^50, 2^51) in a wave that
# takes sq16's two-instruction rounding.  Off the peak steps every delta is far below 2^51, which
# keeps the batch's sum of |delta| below 2^62
WIDE_LOG2_BASE = (0, 3, 6, 9,  10, 10, 10, 10,  8, 8, 8, 8,      12, 13, 14, 15,  11, 11, 11, 11,  10, 11, 12, 13)
WIDE_LOG2_PEAK = (0, 3, 6, 9,  24, 24, 24, 24,  17, 19, 21, 23,  21, 21, 22, 22,  22, 23, 22, 22,  18, 18, 18, 18)


def wide_delta_inputs(S: int = 24, N: int = 16, T: int = 12, seed: int = 31) -> CaseInputs:
    """scenario_batch profiles with a price table per scenario: the default prices of the day times a
    power of two per scenario (an exact scaling of all three prices; larger ones on the two peak
    steps), and alpha = 0.05, so that the first episode's |alpha * r * 2^40| runs from far below 2^51
    to above it.  With the reference's alpha = 1e-5 a delta of 2^51 would need |r| >= 2^11 / 1e-5 =
    2.0e8, whose cost numerator (cost * 15 = r * 60e3 = 1.2e13) lies beyond the 2^40 of the kernels'
    range-free division.  The cases run it without storage: a battery zeroes the net power of most
    agents for the first steps, and with it the cost, so no wave would lie wholly above 2^51."""
    from p2pmicrogrid_amd.dataset import scenario_batch
    from oracle.restatement import prices
    if S != len(WIDE_LOG2_BASE) or T <= max(WIDE_PEAK_STEPS):
        raise ValueError(f"wide_delta_inputs has scales for {len(WIDE_LOG2_BASE)} scenarios and needs T > {max(WIDE_PEAK_STEPS)}")
    inp = scenario_batch(S, N, T, seed=seed)
    time = np.broadcast_to(inp.time, (S, T)).astype(F32)
    log2 = np.repeat(np.asarray(WIDE_LOG2_BASE, np.float64)[:, None], T, axis=1)
    peak = np.asarray(WIDE_LOG2_PEAK, np.float64)
    log2[:, WIDE_PEAK_STEPS[0]] = peak
    log2[:, WIDE_PEAK_STEPS[1]] = np.maximum(peak - 2.0, log2[:, WIDE_PEAK_STEPS[1]])
    scale = np.exp2(log2).astype(F32)
    table = tuple((x * scale).astype(F32) for x in prices(time))
    return CaseInputs(time.copy(), inp.t_out, inp.load_w, inp.pv_w, inp.max_in, inp.t_in0, inp.t_m0, hp_levels_for(S, N),
                      np.full((S, N), BATTERY_J), table, WIDE_ALPHA)


def wave_partition(x: np.ndarray, wave_scenarios: int = 4, bound: float = 2.0 ** 51):
    """x [T, S, N]: per (step, wave of `wave_scenarios` consecutive scenarios) whether every |x| lies
    below `bound` / every |x| lies at or above it; returns (n_below, n_above, n_mixed) over all of them."""
    T, S, N = x.shape
    below = above = mixed = 0
    for s0 in range(0, S, wave_scenarios):
        big = np.abs(x[:, s0:s0 + wave_scenarios]).reshape(T, -1) >= bound
        below += int((~big).all(axis=1).sum())
        above += int(big.all(axis=1).sum())
        mixed += int((big.any(axis=1) & ~big.all(axis=1)).sum())
    return below, above, mixed


def in_wave_below(x: np.ndarray, wave_scenarios: int = 4, bound: float = 2.0 ** 51) -> np.ndarray:
    """x [T, S, N] -> bool [T, S, N]: the values whose whole wave (`wave_scenarios` consecutive scenarios
    at that step) lies below `bound` in magnitude, i.e. the lanes for which a wave-uniform
    `all(|x| < bound)` test holds (sq16's rne_ll takes its two-instruction branch for exactly these)."""
    T, S, N = x.shape
    out = np.zeros(x.shape, bool)
    for s0 in range(0, S, wave_scenarios):
        ok = (np.abs(x[:, s0:s0 + wave_scenarios]).reshape(T, -1) < bound).all(axis=1)
        out[:, s0:s0 + wave_scenarios] = ok[:, None, None]
    return out


def fast_branch_negative_near_bound(x: np.ndarray) -> int:
    """How many x < 0 with |x| in [2^50, 2^51) sit in a wave that lies wholly below 2^51."""
    ax = np.abs(x)
    return int((in_wave_below(x) & (x < 0) & (ax >= 2.0 ** 50) & (ax < 2.0 ** 51)).sum())


def cost_operands_in_fast_range(out, inp: CaseInputs) -> bool:
    """Whether every operand of the cost's division (community.py:56-65: (c * 15) / 60) is 0 or has a
    magnitude in [2^-40, 2^40], the domain of the kernels' range-free quotient (p2pmg_fastmath.h), for
    the oracle's recorded grid and p2p powers and the inputs' prices."""
    buy, inj, p2p = (np.asarray(x, F32).T[:, :, None] for x in inp.prices)  # [T, S, 1]
    g, pp = out["grid"], out["p2p"]
    c = (np.where(g >= 0, g * buy, g * inj).astype(F32) + pp * p2p).astype(F32)
    num = np.abs((c * F32(15)).astype(F32))
    ok = (num == 0) | ((num >= F32(2.0 ** -40)) & (num <= F32(2.0 ** 40)))
    return bool(ok.all())


def rne_exact(x: float) -> int:
    """Round-half-even of a finite double to an integer, in exact rational arithmetic."""
    return round(Fraction(x))  # Python rounds a Fraction half to even


# ----------------------------------------------------------------------------- C. replay codes
def replay_codes(rs: np.random.RandomState, T: int, R: int, S: int, N: int, p_explore: float = 0.4) -> np.ndarray:
    """uint8 [T, R+1, S, N]: about p_explore of the entries an action in {0, 1, 2}, the rest 255 (greedy)."""
    explore = rs.rand(T, R + 1, S, N) < p_explore
    return np.where(explore, rs.randint(0, 3, (T, R + 1, S, N)), 255).astype(np.uint8)


# ----------------------------------------------------------------------------- the two sides
def hp_levels_for(S: int, N: int) -> np.ndarray:
    return np.broadcast_to(np.array([0.0, 1500.0, 3000.0], F32), (S, N, 3)).copy()


def oracle_for(inp: CaseInputs, R: int, q_dtype: str = "f32", battery: bool = True, shared: bool = True) -> OracleBatch:
    S, N = inp.S, inp.N
    par = OracleParams() if inp.alpha is None else OracleParams(alpha=inp.alpha)
    ob = OracleBatch(S=S, N=N, R=R, load_w=inp.load_w, pv_w=inp.pv_w, max_in=inp.max_in, env_time=inp.time,
                     env_tout=inp.t_out, q_dtype=q_dtype, shared_q=shared, hp_levels=inp.hp_levels, params=par,
                     price_table=inp.prices, battery_capacity=inp.capacity.copy() if battery else None)
    ob.t_in, ob.t_m = inp.t_in0.copy(), inp.t_m0.copy()
    return ob


def engine_for(inp: CaseInputs, R: int, q_dtype: str = "f32", battery: bool = True, shared_q=True, scenario_offset: int = 0):
    from p2pmicrogrid_amd.engine import DeviceCommunityBatch
    S, N, T = inp.S, inp.N, inp.T
    kw = {} if inp.alpha is None else {"alpha": inp.alpha}
    eng = DeviceCommunityBatch(S, N, R, T, q_dtype=q_dtype, shared_q=shared_q, scenario_offset=scenario_offset, **kw)
    if inp.prices is None:
        eng.set_env(inp.time, inp.t_out)
    else:
        eng.set_env(inp.time, inp.t_out, *inp.prices)
    eng.set_profiles(inp.load_w, inp.pv_w)
    eng.set_max_in(inp.max_in)
    eng.set_temperatures(inp.t_in0, inp.t_m0)
    eng.set_hp_levels(inp.hp_levels)
    if battery:
        eng.set_battery(inp.capacity, 0.1, 0.9, 0.9)
    return eng
