"""DeviceCommunityBatch — S independent communities x N agents resident in HBM.

This is the batched entry point the reference lacks (SURVEY.md §8b "Add a batched entry
point over S scenarios"): one ``run_episode`` call is one ``CommunityMicrogrid.train_episode``
(community.py:149-182) or ``run`` (community.py:95-123) for every scenario at once, executed
by ONE HIP kernel launch (p2pmg_general.hip::episode_kernel).  The reference-shaped object API
(``community.CommunityMicrogrid`` & co.) is a thin layer over this class with S = 1.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import numpy as np

from . import _lib
from . import setup as cfgmod

F32 = np.float32
RECORD_NAMES = ("reward", "cost", "grid", "p2p", "t_in", "action", "index")
# p2pmg_episode_summary (include/p2pmg.h): the 16 fields in order, and what a launch must record for it
SUMMARY_FIELDS = ("cost", "reward", "grid_import", "grid_export", "p2p_import", "p2p_export", "hp", "load", "pv",
                  "self_consumption", "discomfort_deg", "discomfort_steps", "t_in_min", "t_in_max", "peak_import",
                  "peak_export")
SUMMARY_RECORDS = ("cost", "grid", "p2p", "t_in", "action")  # "reward" is optional (absent: field 1 is 0)


def price_table(time_f32, grid_cost_avg=cfgmod.GRID_COST_AVG, amplitude=cfgmod.GRID_COST_AMPLITUDE,
                period=cfgmod.GRID_COST_PERIOD, phase=cfgmod.GRID_COST_PHASE,
                injection=cfgmod.GRID_INJECTION_PRICE):
    """GridAgent prices per timestep (agent.py:51-67) and the P2P midpoint (community.py:70).

    Host-side table computed once per environment with TF's f32 constant casting; the device
    consumes it as an input (SURVEY.md §3.4 item 1 — TF's Eigen sin is not reproducible).
    """
    t = np.asarray(time_f32, dtype=F32)
    freq = F32(2 * np.pi * cfgmod.HOURS_PER_DAY / period)
    s = np.sin((t * freq) - F32(phase)).astype(F32)
    buy = ((F32(grid_cost_avg) + F32(amplitude) * s) / F32(cfgmod.CENTS_PER_EURO)).astype(F32)
    inj = np.full_like(buy, F32(injection))
    p2p = ((buy + inj) / F32(2)).astype(F32)
    return buy, inj, p2p


def default_policy_map(count: int, n_scenarios: int, n_agents: int) -> np.ndarray:
    """The map agent -> policy of a policy set of ``count`` policies when none is given (p2pmg_set_policy_set
    with policy_of = NULL): int32 [S * N], the identity when count == S * N, a % N (role i of every scenario)
    when count == N, all 0 when count == 1; anything else raises.  Pure NumPy (dqn.default_net_map's twin)."""
    A = int(n_scenarios) * int(n_agents)
    if count == A:
        return np.arange(A, dtype=np.int32)
    if count == n_agents:
        return (np.arange(A) % n_agents).astype(np.int32)
    if count == 1:
        return np.zeros(A, np.int32)
    raise ValueError(f"a policy set of {count} policies needs policy_of: the default maps are for A = {A}, "
                     f"N = {n_agents} or 1 policies")


def snapshot_policy_map(n_snapshots: int, n_days: int, n_agents: int) -> np.ndarray:
    """The map of CommunityMicrogrid.evaluate_policies: K snapshots x D days as S = K * D scenarios, scenario
    k * D + d, agent i on policy k * N + i.  int32 [K * D, N]."""
    k = np.repeat(np.arange(int(n_snapshots), dtype=np.int32), int(n_days))
    return (k[:, None] * np.int32(n_agents) + np.arange(int(n_agents), dtype=np.int32)[None, :]).astype(np.int32)


class DeviceCommunityBatch:
    """Device-resident batch of S communities.  All compute runs in libp2pmg.so."""

    def __init__(self, n_scenarios: int, n_agents: int, rounds: int, horizon: int, q_dtype: str = "f64",
                 device: int = 0, seed: int = 42, scenario_offset: int = 0, shared_q=False, **overrides):
        """shared_q: False (a table per agent of every scenario), True (one table for all) or "role"
        (one table per agent position i, read by agent (s, i) of every scenario s: one community of N
        learners over S scenarios; tables frozen during an episode, updated by apply_q_delta)."""
        self.L = _lib.lib()
        cfg = _lib.default_config()
        cfg.n_scenarios, cfg.n_agents, cfg.rounds, cfg.horizon = n_scenarios, n_agents, rounds, horizon
        cfg.q_dtype = _lib.Q_F64 if q_dtype == "f64" else _lib.Q_F32
        cfg.seed = seed
        cfg.scenario_offset = scenario_offset
        role = isinstance(shared_q, str)
        if role and shared_q != "role":
            raise ValueError(f"shared_q must be False, True or 'role', got {shared_q!r}")
        cfg.shared_q = _lib.SHARED_ROLE if role else int(bool(shared_q))
        for k, v in overrides.items():
            setattr(cfg, k, v)
        self.cfg = cfg
        self.S, self.N, self.R, self.T = n_scenarios, n_agents, rounds, horizon
        self.A = n_scenarios * n_agents
        self.q_dtype = q_dtype
        self.device = device
        self.seed = seed
        self.scenario_offset = scenario_offset
        self.shared_q = "role" if role else bool(shared_q)
        self.n_tables = n_agents if role else (1 if shared_q else self.A)
        self.n_states = cfg.n_time_states * cfg.n_temp_states * cfg.n_balance_states * cfg.n_p2p_states
        self.q_shape = (cfg.n_time_states, cfg.n_temp_states, cfg.n_balance_states, cfg.n_p2p_states,
                        cfg.n_actions)
        ctx = C.c_void_p()
        status = self.L.p2pmg_create(C.byref(cfg), device, C.byref(ctx))
        if status != _lib.P2PMG_OK:
            # a failed create leaves no context: where it gives a reason, that is the calling
            # thread's p2pmg_last_error(NULL)
            raw = self.L.p2pmg_last_error(None) or b""
            msg = "" if raw == b"null context" else raw.decode()
            raise _lib.P2PMGError(f"p2pmg_create: {_lib.STATUS.get(status, status)} {msg}".strip())
        self._ctx = ctx
        self._recorded = 0

    # ----------------------------------------------------------------- lifetime
    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            self.L.p2pmg_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def _chk(self, status, what):
        _lib.check(status, self._ctx, what)

    def sync(self):
        self._chk(self.L.p2pmg_sync(self._ctx), "sync")

    def device_info(self):
        buf = C.create_string_buffer(256)
        mem = C.c_size_t(0)
        self._chk(self.L.p2pmg_device_info(self._ctx, buf, 256, C.byref(mem)), "device_info")
        return buf.value.decode(), mem.value

    # ----------------------------------------------------------------- inputs
    def set_env(self, time, t_out, buy=None, inj=None, p2p=None):
        """Environment rows (environment.py:26-45): time (slot/96) and outdoor temperature,
        shape [T] (shared by all scenarios) or [S, T]."""
        time = np.ascontiguousarray(np.atleast_2d(np.asarray(time, dtype=F32)))
        t_out = np.ascontiguousarray(np.atleast_2d(np.asarray(t_out, dtype=F32)))
        if buy is None:
            buy, inj, p2p = price_table(time)
        arrs = [np.ascontiguousarray(np.atleast_2d(np.asarray(x, dtype=F32))) for x in (buy, inj, p2p)]
        n_env = time.shape[0]
        for x in (time, t_out, *arrs):
            if x.shape != (n_env, self.T):
                raise ValueError(f"env arrays must be [{n_env}, {self.T}], got {x.shape}")
        self._chk(self.L.p2pmg_set_env(self._ctx, n_env, time, t_out, *arrs), "set_env")

    def set_profiles(self, load_w, pv_w):
        """Per-agent power profiles in W, shape [S, N, T] (community.py:219-224)."""
        lw = np.ascontiguousarray(np.asarray(load_w, dtype=F32).reshape(self.A, self.T))
        pw = np.ascontiguousarray(np.asarray(pv_w, dtype=F32).reshape(self.A, self.T))
        self._chk(self.L.p2pmg_set_profiles(self._ctx, lw, pw), "set_profiles")

    def set_max_in(self, max_in):
        m = np.ascontiguousarray(np.asarray(max_in, dtype=F32).reshape(self.A))
        self._chk(self.L.p2pmg_set_agent_params(self._ctx, m), "set_agent_params")

    def set_temperatures(self, t_in, t_m):
        a = np.ascontiguousarray(np.asarray(t_in, dtype=F32).reshape(self.A))
        b = np.ascontiguousarray(np.asarray(t_m, dtype=F32).reshape(self.A))
        self._chk(self.L.p2pmg_set_temperatures(self._ctx, a, b), "set_temperatures")

    def get_temperatures(self):
        a = np.empty(self.A, F32)
        b = np.empty(self.A, F32)
        self._chk(self.L.p2pmg_get_temperatures(self._ctx, a, b), "get_temperatures")
        return a.reshape(self.S, self.N), b.reshape(self.S, self.N)

    def reset_temperatures_philox(self, episode: int, sigma: float = 0.3):
        self._chk(self.L.p2pmg_reset_temperatures_philox(self._ctx, int(episode), float(sigma)), "reset_philox")

    def set_replay_codes(self, codes):
        """uint8 [T, R+1, S, N] (or [T, R+1, N] when S == 1); 255 = greedy."""
        c = np.ascontiguousarray(np.asarray(codes, dtype=np.uint8).reshape(self.T, self.R + 1, self.A))
        self._chk(self.L.p2pmg_set_replay_codes(self._ctx, c.ctypes.data), "set_replay_codes")

    # ----------------------------------------------------------------- Q tables
    def zero_q(self):
        self._chk(self.L.p2pmg_zero_q(self._ctx), "zero_q")

    def get_q(self, first: int = 0, count: Optional[int] = None, dtype=np.float64):
        count = self.n_tables - first if count is None else count
        out = np.empty((count, *self.q_shape), dtype=dtype)
        code = _lib.Q_F64 if np.dtype(dtype) == np.float64 else _lib.Q_F32
        self._chk(self.L.p2pmg_get_q(self._ctx, first, count, out.ctypes.data, code), "get_q")
        return out

    def set_q(self, tables, first: int = 0):
        t = np.asarray(tables)
        dtype = np.float64 if t.dtype == np.float64 else np.float32
        t = np.ascontiguousarray(t.astype(dtype, copy=False).reshape(-1, self.n_states * self.q_shape[-1]))
        code = _lib.Q_F64 if dtype == np.float64 else _lib.Q_F32
        self._chk(self.L.p2pmg_set_q(self._ctx, first, t.shape[0], t.ctypes.data, code), "set_q")

    # ----------------------------------------------------------------- table digests (on the device)
    def _table_range(self, first, count):
        return int(first), int(self.n_tables - first if count is None else count)

    def table_stats(self, first: int = 0, count: Optional[int] = None) -> Dict[str, np.ndarray]:
        """Coverage, value range and greedy-action histogram of tables [first, first + count), reduced
        on the device (p2pmg_table_stats): {"visited": [count] i64, "q_min", "q_max", "abs_max":
        [count] f64, "greedy": [count, n_actions] i64 (visited rows per greedy action)}."""
        first, count = self._table_range(first, count)
        out = np.zeros((max(count, 0), _lib.TABLE_STATS), np.float64)
        self._chk(self.L.p2pmg_table_stats(self._ctx, first, count, out.ctypes.data), "table_stats")
        na = self.q_shape[-1]
        return {"visited": out[:, 0].astype(np.int64), "q_min": out[:, 1].copy(), "q_max": out[:, 2].copy(),
                "abs_max": out[:, 3].copy(), "greedy": out[:, 4:4 + na].astype(np.int64)}

    def greedy_policy(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """u8 [count, n_time, n_temp, n_bal, n_p2p]: each state's greedy action (first maximum, rl.py:116),
        or 255 (_lib.POLICY_UNVISITED) where the row is all zero (p2pmg_greedy_policy)."""
        first, count = self._table_range(first, count)
        out = np.zeros((max(count, 0), *self.q_shape[:-1]), np.uint8)
        self._chk(self.L.p2pmg_greedy_policy(self._ctx, first, count, out.ctypes.data), "greedy_policy")
        return out

    def policy_mark(self):
        """Snapshot every table's packed greedy policy on the device (p2pmg_policy_mark)."""
        self._chk(self.L.p2pmg_policy_mark(self._ctx), "policy_mark")

    def policy_changes(self, first: int = 0, count: Optional[int] = None, remark: bool = True) -> Dict[str, np.ndarray]:
        """{"changed": [count] i64 states whose greedy action differs from the snapshot's, "newly_visited":
        [count] i64 states unvisited in the snapshot and visited now}; remark: the same pass makes the
        current policy of these tables the snapshot (p2pmg_policy_changes)."""
        first, count = self._table_range(first, count)
        ch = np.zeros(max(count, 0), np.int64)
        nv = np.zeros(max(count, 0), np.int64)
        self._chk(self.L.p2pmg_policy_changes(self._ctx, first, count, ch.ctypes.data, nv.ctypes.data,
                                              int(bool(remark))), "policy_changes")
        return {"changed": ch, "newly_visited": nv}

    # ----------------------------------------------------------------- policy sets (packed byte policies)
    def set_policy_set(self, policies=None, policy_of=None, count: Optional[int] = None):
        """The context's policy set (p2pmg_set_policy_set): M packed policies and the map agent -> policy that
        run_policy acts from.  policies: u8 [M, n_states] or [M, n_time, n_temp, n_bal, n_p2p] in greedy_policy's
        order, bytes 0 .. n_actions-1 or 255 (acts as action 0); None: ``count`` empty slots (all 255), for
        capture_policies to fill.  policy_of: int32 [S, N] or [A] with values in [0, M); None: the default
        map (default_policy_map).  count=0 (with policies None) frees the set.  Everything is validated before
        anything is uploaded; a refused call leaves the set as it was.  M * n_states + 4 * A bytes on the device."""
        if policies is None:
            if count is None:
                raise ValueError("set_policy_set needs policies or count")
            M, ptr = int(count), None
        else:
            pol = np.asarray(policies)
            if pol.dtype != np.uint8:
                raise ValueError(f"policies must be uint8, got {pol.dtype}")
            if pol.ndim < 2 or pol.shape[1:] not in ((self.n_states,), tuple(self.q_shape[:-1])):
                raise ValueError(f"policies must be [M, {self.n_states}] or [M, {', '.join(map(str, self.q_shape[:-1]))}], "
                                 f"got {pol.shape}")
            pol = np.ascontiguousarray(pol.reshape(pol.shape[0], self.n_states))
            M, ptr = int(pol.shape[0]), pol.ctypes.data
            if count is not None and int(count) != M:
                raise ValueError(f"count = {count} but {M} policies given")
        mp = None
        if policy_of is not None:
            mp = np.ascontiguousarray(np.asarray(policy_of, dtype=np.int32).reshape(-1))
            if mp.size != self.A:
                raise ValueError(f"policy_of must hold {self.A} entries, got {mp.size}")
        self._chk(self.L.p2pmg_set_policy_set(self._ctx, M, ptr, None if mp is None else mp.ctypes.data), "set_policy_set")

    def policy_set(self):
        """(policies u8 [M, n_time, n_temp, n_bal, n_p2p], policy_of int32 [S, N]) as the device holds them
        (p2pmg_get_policy_set); (None, None) without a set."""
        n = C.c_int(0)
        self._chk(self.L.p2pmg_get_policy_set(self._ctx, C.byref(n), None, None), "get_policy_set")
        if n.value == 0:
            return None, None
        pol = np.empty((n.value, *self.q_shape[:-1]), np.uint8)
        mp = np.empty(self.A, np.int32)
        self._chk(self.L.p2pmg_get_policy_set(self._ctx, C.byref(n), pol.ctypes.data, mp.ctypes.data), "get_policy_set")
        return pol, mp.reshape(self.S, self.N)

    def capture_policies(self, first_table: int = 0, count: Optional[int] = None, first_slot: int = 0):
        """Slot first_slot + k of the policy set becomes greedy_policy() of table first_table + k, on the device
        with no host round trip (p2pmg_policy_set_capture; count None: every table from first_table on)."""
        first_table, count = self._table_range(first_table, count)
        self._chk(self.L.p2pmg_policy_set_capture(self._ctx, first_table, count, int(first_slot)), "policy_set_capture")

    def run_policy(self, record: Sequence[str] = (), kernel: str = "auto"):
        """One greedy episode of every scenario acting from the policy set (p2pmg_run_policy, one launch of
        policy_episode_kernel): agent a takes policies[policy_of[a]][state] wherever a greedy run_episode would
        take the argmax of its Q row; everything else, records included, is that episode bit for bit.
        kernel: 'auto' | 'tile' (the LDS-tile form at any N, as in run_episode)."""
        mask = 0
        for r in record:
            mask |= _lib.REC[r]
        flags = {"auto": 0, "tile": _lib.FLAG_TILE_KERNEL}[kernel]
        if flags:
            self._chk(self.L.p2pmg_run_policy_ex(self._ctx, mask, flags), "run_policy")
        else:
            self._chk(self.L.p2pmg_run_policy(self._ctx, mask), "run_policy")
        self._recorded = mask

    # ----------------------------------------------------------------- sparse table checkpoints
    def sparse_count(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """int64 [count]: the stored rows of tables [first, first + count), rows with a non-zero bit in
        one of their n_actions entries (p2pmg_sparse_count; -0.0 counts, unlike table_stats' visited)."""
        first, count = self._table_range(first, count)
        out = np.zeros(max(count, 0), np.int64)
        self._chk(self.L.p2pmg_sparse_count(self._ctx, first, count, out.ctypes.data), "sparse_count")
        return out

    def get_q_sparse(self, first: int = 0, count: Optional[int] = None, dtype=None) -> Dict[str, np.ndarray]:
        """The sparse form of tables [first, first + count), compacted on the device (p2pmg_get_q_sparse):
        {"shape": q_shape int64 [5], "offsets": int64 [count + 1], "rows": int32 [total] state indices of the
        stored rows, ascending inside each table, "values": [total, n_actions]}; table k's rows are
        rows[offsets[k]:offsets[k + 1]].  dtype None: the tables' own (then bit for bit)."""
        first, count = self._table_range(first, count)
        dt = np.dtype((np.float64 if self.q_dtype == "f64" else np.float32) if dtype is None else dtype)
        if dt not in (np.float64, np.float32):
            raise ValueError(f"dtype must be float64 or float32, got {dt}")
        n_rows = self.sparse_count(first, count)
        total = int(n_rows.sum())
        rows = np.empty(total, np.int32)
        values = np.empty((total, self.q_shape[-1]), dt)
        self._chk(self.L.p2pmg_get_q_sparse(self._ctx, first, count, total, n_rows.ctypes.data, rows.ctypes.data,
                                            values.ctypes.data, _lib.Q_F64 if dt == np.float64 else _lib.Q_F32),
                  "get_q_sparse")
        offsets = np.zeros(max(count, 0) + 1, np.int64)
        np.cumsum(n_rows, out=offsets[1:])
        return {"shape": np.asarray(self.q_shape, np.int64), "offsets": offsets, "rows": rows, "values": values}

    def set_q_sparse(self, sparse, first: int = 0, zero: bool = True):
        """Write a sparse form's tables over tables [first, first + its count) by a scatter on the device
        (p2pmg_set_q_sparse).  zero: those tables are zeroed first, so that they become the form's tables;
        else only the listed rows are overwritten.  ValueError for a form of another table shape; what the
        library refuses (unsorted, duplicated or out-of-range indices) leaves the tables unchanged."""
        from .rl import SPARSE_KEYS
        missing = [k for k in SPARSE_KEYS if k not in sparse]
        if missing:
            raise ValueError(f"not a sparse table form: no {missing}")
        shape = tuple(int(x) for x in np.asarray(sparse["shape"]).reshape(-1))
        if shape != tuple(self.q_shape):
            raise ValueError(f"sparse form holds tables of shape {shape}, this context {tuple(self.q_shape)}")
        offsets = np.ascontiguousarray(sparse["offsets"], np.int64).reshape(-1)
        rows = np.ascontiguousarray(sparse["rows"], np.int32).reshape(-1)
        values = np.asarray(sparse["values"])
        values = np.ascontiguousarray(values, values.dtype if values.dtype in (np.float64, np.float32) else np.float64)
        if offsets.size < 1 or offsets[0] != 0 or offsets[-1] != rows.size or values.shape != (rows.size, shape[-1]):
            raise ValueError("sparse form: offsets, rows and values do not belong together")
        n_rows = np.ascontiguousarray(np.diff(offsets))
        code = _lib.Q_F64 if values.dtype == np.float64 else _lib.Q_F32
        self._chk(self.L.p2pmg_set_q_sparse(self._ctx, int(first), n_rows.size, n_rows.ctypes.data, rows.ctypes.data,
                                            values.ctypes.data, code, int(bool(zero))), "set_q_sparse")

    def copy_q(self, src: int, first: int, count: int):
        """Tables [first, first + count) become bit copies of table src, on the device (p2pmg_copy_q)."""
        self._chk(self.L.p2pmg_copy_q(self._ctx, int(src), int(first), int(count)), "copy_q")

    def save_tables(self, path: str, first: int = 0, count: Optional[int] = None) -> str:
        """Tables [first, first + count) as one uncompressed .npz with the four keys of get_q_sparse, in
        the tables' own dtype; returns the path written (".npz" appended where missing)."""
        from .rl import save_sparse_file
        return save_sparse_file(path, self.get_q_sparse(first, count))

    def load_tables(self, path: str, first: int = 0) -> int:
        """The tables of a save_tables file over tables [first, first + its count) (np.load with
        allow_pickle=False); ValueError where the file's table shape is not this context's.  Returns
        the number of tables loaded."""
        from .rl import load_sparse_file
        sparse = load_sparse_file(path, self.q_shape)
        self.set_q_sparse(sparse, first=first, zero=True)
        return int(sparse["offsets"].size - 1)

    # ----------------------------------------------------------------- heterogeneous agents / storage
    def set_hp_levels(self, levels):
        """Per-agent heat-pump power of actions 0..2 in W, [S, N, 3] (0 for agents without one)."""
        lv = np.ascontiguousarray(np.asarray(levels, dtype=F32).reshape(self.A, 3))
        self._chk(self.L.p2pmg_set_hp_levels(self._ctx, lv), "set_hp_levels")

    def get_hp_levels(self) -> np.ndarray:
        """[S, N, 3] f32: the heat-pump power per action the kernels read."""
        out = np.empty((self.A, 3), F32)
        self._chk(self.L.p2pmg_get_hp_levels(self._ctx, out), "get_hp_levels")
        return out.reshape(self.S, self.N, 3)

    def set_thermal(self, setpoint, cop=None, lower=None, upper=None):
        """Per-agent comfort setpoint and heat-pump COP (HPHeating / HeatPump, heating.py:92-130):
        [S, N] arrays or scalars.  lower / upper default to the reference's bounds, formed in f64
        and cast afterwards: f32(float64(setpoint) -/+ 1.0) (heating.py:92-94).  cop None: the
        config's.  set_thermal(None) restores the config's values for every agent."""
        if setpoint is None:
            self._chk(self.L.p2pmg_set_thermal(self._ctx, None), "set_thermal")
            return
        def per_agent(x):
            return np.broadcast_to(np.asarray(x, np.float64), (self.S, self.N)).reshape(self.A)
        sp = per_agent(setpoint)
        margin = float(self.cfg.temp_margin)  # HPHeating.TEMPERATURE_MARGIN = 1
        par = np.empty((self.A, 4), F32)
        par[:, 0] = sp.astype(F32)
        par[:, 1] = (sp - margin).astype(F32) if lower is None else per_agent(lower).astype(F32)
        par[:, 2] = (sp + margin).astype(F32) if upper is None else per_agent(upper).astype(F32)
        par[:, 3] = F32(self.cfg.hp_cop) if cop is None else per_agent(cop).astype(F32)
        self._chk(self.L.p2pmg_set_thermal(self._ctx, par.ctypes.data), "set_thermal")

    def get_thermal(self) -> np.ndarray:
        """[S, N, 4] f32 {setpoint, lower bound, upper bound, COP} the kernels read."""
        out = np.empty((self.A, 4), F32)
        self._chk(self.L.p2pmg_get_thermal(self._ctx, out), "get_thermal")
        return out.reshape(self.S, self.N, 4)

    def set_learning(self, alpha=None, gamma=None, penalty_weight=None):
        """Per-agent learner constants: each QActor's own alpha and gamma (rl.py:58-71) and the comfort
        weight of the agent's reward (agent.py:225-232).  Scalars or anything that broadcasts to
        [S, N]; None keeps the config's value for that field, and set_learning() restores the
        config's values for every agent."""
        def per_agent(x, dt):
            if x is None:
                return None
            x = np.asarray(x, dt)
            try:
                return np.ascontiguousarray(np.broadcast_to(x, (self.S, self.N)).reshape(self.A))
            except ValueError:
                raise ValueError(f"learning arrays must broadcast to [{self.S}, {self.N}], got {x.shape}") from None
        a, g, w = per_agent(alpha, np.float64), per_agent(gamma, np.float64), per_agent(penalty_weight, F32)
        self._chk(self.L.p2pmg_set_learning(self._ctx, *(None if x is None else x.ctypes.data for x in (a, g, w))),
                  "set_learning")

    def get_learning(self) -> Dict[str, np.ndarray]:
        """{"alpha": [S, N] f64, "gamma": [S, N] f64, "penalty_weight": [S, N] f32} the kernels read."""
        a, g, w = np.empty(self.A, np.float64), np.empty(self.A, np.float64), np.empty(self.A, F32)
        self._chk(self.L.p2pmg_get_learning(self._ctx, a.ctypes.data, g.ctypes.data, w.ctypes.data), "get_learning")
        shape = (self.S, self.N)
        return {"alpha": a.reshape(shape), "gamma": g.reshape(shape), "penalty_weight": w.reshape(shape)}

    def set_battery(self, capacity=None, min_soc=0.1, max_soc=0.9, efficiency=0.9, soc0=None):
        """Battery per agent (capacity [S, N] in J, 0 = none); None disables storage."""
        if capacity is None:
            self._chk(self.L.p2pmg_set_battery(self._ctx, None, 0.1, 0.9, 1.0, None), "set_battery")
            return
        def per_agent(x):
            x = np.asarray(x, np.float64)
            return np.ascontiguousarray(x.reshape(self.A) if x.size == self.A else np.broadcast_to(x, (self.A,)))
        cap = per_agent(capacity)
        s0 = None if soc0 is None else per_agent(soc0)
        self._chk(self.L.p2pmg_set_battery(self._ctx, cap.ctypes.data, float(min_soc), float(max_soc),
                                           float(efficiency), None if s0 is None else s0.ctypes.data), "set_battery")

    def get_soc(self):
        out = np.empty(self.A, np.float64)
        self._chk(self.L.p2pmg_get_soc(self._ctx, out.ctypes.data), "get_soc")
        return out.reshape(self.S, self.N)

    def battery_seq(self, balance, soc, capacity, min_soc=0.1, max_soc=0.9, efficiency=0.9):
        """Battery rule (agent.py:138-153) over per-agent sequences [agents, steps] on the device."""
        b = np.ascontiguousarray(np.atleast_2d(np.asarray(balance, np.float64)))
        ag, st = b.shape
        ob = np.empty_like(b)
        sh = np.empty_like(b)
        s_ = np.ascontiguousarray(np.broadcast_to(np.asarray(soc, np.float64), (ag,))).copy()
        cap = np.ascontiguousarray(np.broadcast_to(np.asarray(capacity, np.float64), (ag,)))
        self._chk(self.L.p2pmg_battery_seq(self._ctx, ag, st, b.ctypes.data, ob.ctypes.data, sh.ctypes.data,
                                           s_.ctypes.data, cap.ctypes.data, float(min_soc), float(max_soc),
                                           float(efficiency)), "battery_seq")
        return ob, sh, s_

    # ----------------------------------------------------------------- shared policy table
    def apply_q_delta(self):
        self._chk(self.L.p2pmg_apply_q_delta(self._ctx), "apply_q_delta")

    def get_q_delta(self):
        """int64 fixed-point (2^-40) deltas in q_shape; with per-role tables [N, *q_shape]."""
        if self.shared_q == "role":
            out = np.empty((self.N, *self.q_shape), np.int64)
        else:
            out = np.empty(self.q_shape, np.int64)
        self._chk(self.L.p2pmg_get_q_delta(self._ctx, out.ctypes.data), "get_q_delta")
        return out

    def set_q_delta(self, delta):
        rows = self.n_states * (self.N if self.shared_q == "role" else 1)
        d = np.ascontiguousarray(np.asarray(delta, np.int64).reshape(rows, self.q_shape[-1]))
        self._chk(self.L.p2pmg_set_q_delta(self._ctx, d.ctypes.data), "set_q_delta")

    def comm_init(self, unique_id: bytes, rank: int, nranks: int):
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self._chk(self.L.p2pmg_comm_init(self._ctx, buf, rank, nranks), "comm_init")

    def allreduce_q_delta(self):
        self._chk(self.L.p2pmg_allreduce_q_delta(self._ctx), "allreduce_q_delta")

    def comm_nranks(self) -> int:
        """Ranks of the RCCL communicator (1 without one)."""
        n = C.c_int(0)
        self._chk(self.L.p2pmg_comm_nranks(self._ctx, C.byref(n)), "comm_nranks")
        return int(n.value)

    def allreduce_metrics(self):
        """(sum of the last episode's rewards over every rank's scenarios, scenario count): the
        local sum on the device, then an RCCL all-reduce when a communicator exists."""
        out = np.zeros(2, np.float64)
        self._chk(self.L.p2pmg_allreduce_metrics(self._ctx, out.ctypes.data), "allreduce_metrics")
        return float(out[0]), int(out[1])

    def table_hash_allgather(self) -> np.ndarray:
        """64-bit fingerprints of every rank's Q-table replica, in rank order (RCCL all-gather)."""
        out = np.zeros(max(1, self.comm_nranks()), np.uint64)
        self._chk(self.L.p2pmg_table_hash_allgather(self._ctx, out.ctypes.data), "table_hash_allgather")
        return out

    # ----------------------------------------------------------------- the hot path
    def run_episode(self, mode: str = "train", rng: str = "replay", episode: int = 0, epsilon=0.81,
                    record: Sequence[str] = (), philox: str = "auto", kernel: str = "auto",
                    scen_per_wave: int = 0, reset_sigma: Optional[float] = None,
                    next_epsilon: Optional[float] = None):
        """Launch one episode for all scenarios (asynchronous; stream-ordered).
        philox: 'auto' | 'prepass' | 'inkernel' placement of the Philox draws.
        kernel: 'auto' (the fast per-agent-table kernel whenever it applies) | 'general' | 'tile'
            (the general kernel's LDS-tile form, which every N outside {1..8, 16} runs, at any N).
        scen_per_wave: fast kernel only, scenarios per 64-lane wave (0 = full waves).
        reset_sigma: end the episode with agent.reset() (community.py:181), i.e. exactly
        reset_temperatures_philox(episode + 1, reset_sigma), fused into the episode launch.
        next_epsilon: the next episode's epsilon when the caller knows its decay schedule
        (community.py:279-286), so that the speculative pre-pass this launch writes for
        episode + 1 is a hit (None: the same epsilon).
        epsilon: a float, or [S] for one epsilon per scenario (Philox training only; the launch is
        then run_episodes(episode, epsilon[None, :]), without a speculative pre-pass)."""
        if np.ndim(epsilon) != 0:
            eps = np.asarray(epsilon, np.float64)
            if eps.shape != (self.S,):
                raise ValueError(f"epsilon must be a float or [{self.S}], got {eps.shape}")
            if mode != "train" or rng != "philox":
                raise ValueError("per-scenario epsilon needs mode='train' and rng='philox'")
            return self.run_episodes(episode, eps[None, :], reset_sigma=reset_sigma, scen_per_wave=scen_per_wave,
                                     record=record, philox=philox, kernel=kernel)
        mask = 0
        for r in record:
            mask |= _lib.REC[r]
        flags = {"auto": 0, "prepass": _lib.FLAG_PHILOX_PREPASS, "inkernel": _lib.FLAG_PHILOX_INKERNEL}[philox]
        flags |= {"auto": 0, "general": _lib.FLAG_GENERAL_KERNEL, "tile": _lib.FLAG_TILE_KERNEL}[kernel]
        if reset_sigma is not None:
            flags |= _lib.FLAG_RESET_T0
        if next_epsilon is not None:  # a guess of 0.0 is a real guess (P2PMG_FLAG_NEXT_EPSILON)
            flags |= _lib.FLAG_NEXT_EPSILON
        args = _lib.EpisodeArgs(_lib.MODE_TRAIN if mode == "train" else _lib.MODE_GREEDY,
                                _lib.RNG_REPLAY if rng == "replay" else _lib.RNG_PHILOX,
                                int(episode), mask, float(epsilon), flags, int(scen_per_wave),
                                float(reset_sigma or 0.0), float(next_epsilon or 0.0))
        self._chk(self.L.p2pmg_run_episode(self._ctx, C.byref(args)), "run_episode")
        self._recorded = mask

    def run_episodes(self, episode: int, epsilons, reset_sigma: Optional[float] = None,
                     next_epsilons=None, scen_per_wave: int = 0, record: Sequence[str] = (), philox: str = "auto",
                     kernel: str = "auto"):
        """Train len(epsilons) consecutive episodes with Philox draws (community.py:279-286's loop
        body): episode + k at epsilons[k], each ending with the T0 reset when reset_sigma is given.
        Where the fast kernel applies, chained launches run up to 64 episodes each, every wave
        going through its episodes back to back; results are those of run_episode per episode,
        bit for bit.  next_epsilons: the next call's epsilons (its speculative pre-pass).  record:
        what the last episode leaves in the record buffers (as after run_episode per episode).
        epsilons [n, S]: scenario s explores at epsilons[k, s] in episode + k (p2pmg_run_episodes_eps;
        next_epsilons is ignored: the call does not speculate).  philox / kernel: as in run_episode."""
        eps = np.ascontiguousarray(epsilons, dtype=np.float64)
        if eps.ndim > 2 or (eps.ndim == 2 and eps.shape[1] != self.S) or eps.size == 0:
            raise ValueError(f"epsilons must be [n] or [n, {self.S}], got {eps.shape}")
        flags = _lib.FLAG_RESET_T0 if reset_sigma is not None else 0
        flags |= {"auto": 0, "prepass": _lib.FLAG_PHILOX_PREPASS, "inkernel": _lib.FLAG_PHILOX_INKERNEL}[philox]
        flags |= {"auto": 0, "general": _lib.FLAG_GENERAL_KERNEL, "tile": _lib.FLAG_TILE_KERNEL}[kernel]
        mask = 0
        for r in record:
            mask |= _lib.REC[r]
        if eps.ndim == 2:
            args = _lib.EpisodeArgs(_lib.MODE_TRAIN, _lib.RNG_PHILOX, int(episode), mask, 0.0, flags,
                                    int(scen_per_wave), float(reset_sigma or 0.0), 0.0)
            self._chk(self.L.p2pmg_run_episodes_eps(self._ctx, C.byref(args), int(eps.shape[0]), eps),
                      "run_episodes_eps")
            self._recorded = mask
            self._chain_len = int(eps.shape[0])
            return
        eps = eps.reshape(-1)
        args = _lib.EpisodeArgs(_lib.MODE_TRAIN, _lib.RNG_PHILOX, int(episode), mask, float(eps[0]), flags,
                                int(scen_per_wave), float(reset_sigma or 0.0), 0.0)
        nxt = None if next_epsilons is None else np.ascontiguousarray(next_epsilons, dtype=np.float64).reshape(-1)
        self._chain_eps = (eps, nxt)  # kept alive for the call
        self._chk(self.L.p2pmg_run_episodes(self._ctx, C.byref(args), int(eps.size), eps,
                                            0 if nxt is None else int(nxt.size),
                                            None if nxt is None else nxt.ctypes.data), "run_episodes")
        self._recorded = mask
        self._chain_len = int(eps.size)

    def episode_rewards(self) -> np.ndarray:
        """[n, S] episode rewards (community.py:179) of every episode of the last run_episodes."""
        n = getattr(self, "_chain_len", 0)
        out = np.empty((n, self.S), F32)
        self._chk(self.L.p2pmg_get_episode_rewards(self._ctx, n, out), "get_episode_rewards")
        return out

    def run_rule_episode(self, record: Sequence[str] = ()):
        """CommunityMicrogrid.run of a RuleAgent community (community.py:95-123, 237-238; agent.py:106-136):
        hysteresis heat pumps, no policy, R = 0.  Records: cost, grid, p2p, t_in, action (0 off, 2 on)."""
        mask = 0
        for r in record:
            mask |= _lib.REC[r]
        self._chk(self.L.p2pmg_run_rule_episode(self._ctx, mask), "run_rule_episode")
        self._recorded = mask

    def set_hp_state(self, on):
        """RuleAgent HeatPump.power per agent (0/1), [S, N]."""
        a = np.ascontiguousarray(np.asarray(on, dtype=F32).reshape(self.A))
        self._chk(self.L.p2pmg_set_hp_state(self._ctx, a), "set_hp_state")

    def get_hp_state(self) -> np.ndarray:
        out = np.empty(self.A, F32)
        self._chk(self.L.p2pmg_get_hp_state(self._ctx, out), "get_hp_state")
        return out.reshape(self.S, self.N)

    def prepass_stats(self):
        """(hits, misses): fast-path launches whose step pre-pass the previous launch had produced
        beside its own episode, and launches that had to run it themselves."""
        h, m = C.c_int64(0), C.c_int64(0)
        self._chk(self.L.p2pmg_prepass_stats(self._ctx, C.byref(h), C.byref(m)), "prepass_stats")
        return int(h.value), int(m.value)

    def chain_lag(self):
        """(D, safe): the hazard distance of the uploaded inputs and whether chained launches may run two
        episodes per wave (D + 4 <= T / 2; p2pmg_chain_lag).  Known after the first run_episodes since
        the last upload; D = -1 where it is not computed (T > 512)."""
        d, ok = C.c_int(0), C.c_int(0)
        self._chk(self.L.p2pmg_chain_lag(self._ctx, C.byref(d), C.byref(ok)), "chain_lag")
        return int(d.value), bool(ok.value)

    def last_kernel(self) -> str:
        """Name of the kernel the last episode launch ran (fast or general path)."""
        return (self.L.p2pmg_last_kernel(self._ctx) or b"").decode()

    def last_kernel_ms(self) -> float:
        ms = C.c_float(0)
        self._chk(self.L.p2pmg_last_kernel_ms(self._ctx, C.byref(ms)), "last_kernel_ms")
        return float(ms.value)

    def kernel_times(self, max_n: int = 4096) -> np.ndarray:
        """HIP-event durations (ms) of the episode kernels since the last reset (syncs)."""
        out = np.empty(max_n, F32)
        n = C.c_int(0)
        self._chk(self.L.p2pmg_kernel_times(self._ctx, out, max_n, C.byref(n)), "kernel_times")
        return out[:n.value].copy()

    def collective_ms(self):
        """(total ms, count) of the data-path RCCL collectives (shared-table delta all-reduce, DQN
        gradient-segment all-gather) since the last reset_kernel_times, every call counted (HIP
        events on the context's stream; syncs)."""
        ms, n = C.c_double(0.0), C.c_int(0)
        self._chk(self.L.p2pmg_collective_ms(self._ctx, C.byref(ms), C.byref(n)), "collective_ms")
        return float(ms.value), int(n.value)

    def reset_kernel_times(self):
        self._chk(self.L.p2pmg_reset_kernel_times(self._ctx), "reset_kernel_times")

    def set_timing_period(self, period: int):
        """Stamp timing events on every period-th episode launch only (timing-only setting)."""
        self._chk(self.L.p2pmg_set_timing_period(self._ctx, int(period)), "set_timing_period")

    def get_record(self, name: str) -> np.ndarray:
        """[T, S, N] for per-step records, [T, R+1, S, N] for action/index."""
        bit = _lib.REC[name]
        if name in ("action", "index"):
            shape = (self.T, self.R + 1, self.S, self.N)
            dt = np.uint8 if name == "action" else np.int32
        else:
            shape = (self.T, self.S, self.N)
            dt = np.float32
        out = np.empty(shape, dtype=dt)
        self._chk(self.L.p2pmg_get_record(self._ctx, bit, out.ctypes.data), f"get_record({name})")
        return out

    def get_records(self, names: Sequence[str]) -> Dict[str, np.ndarray]:
        return {n: self.get_record(n) for n in names}

    def episode_summary(self, kwh: bool = False) -> Dict[str, Dict[str, np.ndarray]]:
        """The last episode launch's records reduced over time on the device (p2pmg_episode_summary):
        {"agent": {name: [S, N] f64}, "scenario": {name: [S] f64}} for the names in SUMMARY_FIELDS.
        The launch must have recorded SUMMARY_RECORDS.  Energies (fields 2-9) are in W-steps;
        kwh=True multiplies them by time_slot / 60 * 1e-3.  The peaks stay in W."""
        nf = len(SUMMARY_FIELDS)
        ag = np.empty((self.A, nf), np.float64)
        sc = np.empty((self.S, nf), np.float64)
        self._chk(self.L.p2pmg_episode_summary(self._ctx, ag.ctypes.data, sc.ctypes.data), "episode_summary")
        if kwh:
            k = float(self.cfg.time_slot) / 60.0 * 1e-3
            ag[:, 2:10] *= k
            sc[:, 2:10] *= k
        ag = ag.reshape(self.S, self.N, nf)
        return {"agent": {n: np.ascontiguousarray(ag[..., j]) for j, n in enumerate(SUMMARY_FIELDS)},
                "scenario": {n: np.ascontiguousarray(sc[:, j]) for j, n in enumerate(SUMMARY_FIELDS)}}

    def day_profile(self, period: Optional[int] = None, steps: Optional[Sequence[int]] = None,
                    scenarios: Optional[Sequence[int]] = None, groups=None, n_groups: Optional[int] = None,
                    as_dict: bool = False, kwh: bool = False):
        """The last episode launch's records reduced over scenarios on the device (p2pmg_day_profile):
        (sums [G, P, N, 16] i64, extrema [G, P, N, 8] f32, com_sums [G, P, 4] i64, com_extrema [G, P, 2] f32),
        bit for bit day_profile.from_records of the same records, so day_profile.merge and
        distributed.merge_day_profiles take them as they are.  Arguments as from_records': period None or 0 = T
        (no folding); steps, scenarios = (first, stop), None = all; groups [S] labels in [-1, n_groups), None =
        one group; n_groups None = max(label) + 1.  The launch must have recorded SUMMARY_RECORDS.
        as_dict=True: day_profile.as_dict of the arrays, kwh=True with the mean powers as kWh per step."""
        from . import day_profile as dayprof
        t0, n_t = (0, -1) if steps is None else (int(steps[0]), int(steps[1]) - int(steps[0]))
        s0, n_s = (0, -1) if scenarios is None else (int(scenarios[0]), int(scenarios[1]) - int(scenarios[0]))
        if n_t < 0 and steps is not None or n_s < 0 and scenarios is not None:
            raise ValueError("day_profile: a range's stop lies before its first")
        lab = None
        if groups is not None:
            lab = np.ascontiguousarray(np.asarray(groups).astype(np.int64).reshape(-1))
            if lab.shape != (self.S,):
                raise ValueError("day_profile: one label per scenario")
            lab = np.clip(lab, -2, np.iinfo(np.int32).max).astype(np.int32)  # the library refuses what lies outside [-1, G)
        args = _lib.DayProfileArgs(int(period or 0), t0, n_t, s0, n_s, 0 if n_groups is None else max(int(n_groups), 1),
                                   None if lab is None else lab.ctypes.data)
        G, P = C.c_int32(0), C.c_int32(0)
        self._chk(self.L.p2pmg_day_profile_shape(self._ctx, C.byref(args), C.byref(G), C.byref(P)), "day_profile")
        G, P = int(G.value), int(P.value)
        out = (np.empty((G, P, self.N, 16), np.int64), np.empty((G, P, self.N, 8), F32), np.empty((G, P, 4), np.int64),
               np.empty((G, P, 2), F32))
        self._chk(self.L.p2pmg_day_profile(self._ctx, C.byref(args), *(a.ctypes.data for a in out)), "day_profile")
        if not as_dict:
            return out
        return dayprof.as_dict(*out, energy_scale=float(self.cfg.time_slot) / 60.0 * 1e-3 if kwh else 1.0)

    def episode_reward(self) -> np.ndarray:
        out = np.empty(self.S, F32)
        self._chk(self.L.p2pmg_get_episode_reward(self._ctx, out), "episode_reward")
        return out

    # ----------------------------------------------------------------- primitives
    def rc_step(self, t_out, t_in, t_m, hp, cop=None, solar_gain=0.0):
        """Batched heating.temperature_simulation (heating.py:37-56) on the device.
        cop: per-element COP (None: the config's); solar_gain: f32(gA * solar_rad).  With either
        given the call is p2pmg_rc_step_ex, else p2pmg_rc_step."""
        ins = (t_out, t_in, t_m, hp) if cop is None else (t_out, t_in, t_m, hp, cop)
        arrs = [np.ascontiguousarray(np.asarray(x, dtype=F32).ravel()) for x in np.broadcast_arrays(*ins)]
        n = arrs[0].size
        a = np.empty(n, F32)
        b = np.empty(n, F32)
        if cop is None and float(solar_gain) == 0.0:
            self._chk(self.L.p2pmg_rc_step(self._ctx, n, *arrs, a, b), "rc_step")
        else:
            self._chk(self.L.p2pmg_rc_step_ex(self._ctx, n, *arrs[:4], None if cop is None else arrs[4].ctypes.data,
                                              F32(solar_gain), a, b), "rc_step_ex")
        shape = np.broadcast(*ins).shape
        return a.reshape(shape), b.reshape(shape)

    def fdiv_check(self, a, b):
        """The kernels' fast f32 quotients of a / b and the IEEE one: [n, 4] (p2pmg_fdiv_check)."""
        a = np.ascontiguousarray(np.asarray(a, F32).ravel())
        b = np.ascontiguousarray(np.asarray(b, F32).ravel())
        out = np.empty((a.size, 4), F32)
        self._chk(self.L.p2pmg_fdiv_check(self._ctx, a.size, a.ctypes.data, b.ctypes.data, out.ctypes.data), "fdiv_check")
        return out

    def fdiv64_check(self, a, b):
        """The kernels' fast f64 quotients and the IEEE one: [n, 3] (p2pmg_fdiv64_check)."""
        a = np.ascontiguousarray(np.asarray(a, np.float64).ravel())
        b = np.ascontiguousarray(np.asarray(b, np.float64).ravel())
        out = np.empty((a.size, 3), np.float64)
        self._chk(self.L.p2pmg_fdiv64_check(self._ctx, a.size, a.ctypes.data, b.ctypes.data, out.ctypes.data),
                  "fdiv64_check")
        return out

    def state_indices(self, obs):
        """Batched QActor._get_state_indices (rl.py:89-95) on the device; obs [..., 4]."""
        o = np.ascontiguousarray(np.asarray(obs, dtype=F32).reshape(-1, 4))
        idx = np.empty(o.shape, np.int32)
        self._chk(self.L.p2pmg_state_indices(self._ctx, o.shape[0], o, idx.ctypes.data), "state_indices")
        return idx.reshape(np.shape(obs))


def _q_calls(eng: "DeviceCommunityBatch", agents, s_obs, codes, rewards=None, ns_obs=None, train=False):
    agents = np.ascontiguousarray(np.asarray(agents, dtype=np.int32).ravel())
    n = agents.size
    s_obs = np.ascontiguousarray(np.asarray(s_obs, dtype=F32).reshape(n, 4))
    codes = np.ascontiguousarray(np.asarray(codes, dtype=np.uint8).ravel())
    acts = np.empty(n, np.int32)
    qv = np.empty(n, np.float64)
    if train:
        rewards = np.ascontiguousarray(np.asarray(rewards, dtype=F32).ravel())
        ns_obs = np.ascontiguousarray(np.asarray(ns_obs, dtype=F32).reshape(n, 4))
    eng._chk(eng.L.p2pmg_q_calls(eng._ctx, n, agents.ctypes.data, s_obs.ctypes.data, codes.ctypes.data,
                                 rewards.ctypes.data if train else None, ns_obs.ctypes.data if train else None,
                                 int(bool(train)), acts.ctypes.data, qv.ctypes.data), "q_calls")
    return acts, qv


DeviceCommunityBatch.q_calls = _q_calls


def comm_unique_id() -> bytes:
    """ncclGetUniqueId through libp2pmg (RCCL loaded at run time); rank 0 shares it."""
    buf = (C.c_uint8 * 128)()
    _lib.check(_lib.lib().p2pmg_comm_unique_id(buf), what="comm_unique_id")
    return bytes(buf)


def unpack_index(packed: np.ndarray) -> np.ndarray:
    """P2PMG_REC_INDEX packing -> [..., 4] (it, iT, ib, ip)."""
    p = np.asarray(packed, dtype=np.int64)
    return np.stack([p & 0xFF, (p >> 8) & 0xFF, (p >> 16) & 0xFF, (p >> 24) & 0xFF], axis=-1)
