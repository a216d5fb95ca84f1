"""DeviceDQNBatch — the DQN variant (BASELINE.json configs[4]) of the batched community.

S scenarios x N ``DQNAgent``s (agent.py:301-350) resident in HBM: per agent (or ONE shared
network, the data-parallel config 5) an online and a target ``QNetwork`` (rl.py:135-148,
5 -> 64 -> 64 -> 1 ReLU), Adam state and a replay ring of 5000 transitions (rl.py:200-248).
One ``run_episode`` call runs T environment steps on the device; each step is an act launch
(negotiation rounds with the Q-MLP, market, reward, memory append, RC update) followed in
TRAIN mode by the train launch (sample 32, target/online forward + backward on f32 MFMA,
clip, Adam, soft update; p2pmg_dqn_*.hip).

    mode 'fill'   CommunityMicrogrid.init_buffers (community.py:125-147): act + remember
    mode 'train'  CommunityMicrogrid.train_episode (community.py:149-182) with DQNAgent.train
    mode 'greedy' CommunityMicrogrid.run (community.py:95-123)

Weights use the Keras ``trainable_weights`` order packed into 4609 floats:
W1[5][64] | b1[64] | W2[64][64] | b2[64] | W3[64][1] | b3[1].
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import numpy as np

from . import _lib
from .engine import DeviceCommunityBatch

F32 = np.float32
N_PARAMS = _lib.DQN_PARAMS
WHICH = {"online": _lib.DQN_ONLINE, "target": _lib.DQN_TARGET, "adam_m": _lib.DQN_ADAM_M, "adam_v": _lib.DQN_ADAM_V}
MAP_WHICH = {"online": _lib.DQN_ONLINE, "target": _lib.DQN_TARGET}  # arrays the policy map reads
EVAL_SOURCES = {"online": _lib.DQN_ONLINE, "target": _lib.DQN_TARGET, "policy": _lib.DQN_POLICY_SET}  # run_greedy
MODES = {"train": _lib.MODE_TRAIN, "greedy": _lib.MODE_GREEDY, "fill": _lib.MODE_FILL}
ACTION_VALUES = np.array([0.0, 0.5, 1.0], dtype=F32)  # ActorModel.actions rl.py:153


def glorot_init(n_nets: int, seed: int = 0) -> np.ndarray:
    """Keras Dense defaults in distribution (glorot_uniform kernels, zero biases) from a NumPy
    seed.  TF's own initialiser stream cannot be reproduced without TF."""
    rs = np.random.RandomState(seed)
    th = np.zeros((n_nets, N_PARAMS), dtype=F32)
    off = 0
    for fi, fo in ((5, 64), (64, 64), (64, 1)):
        lim = np.sqrt(6.0 / (fi + fo))
        th[:, off:off + fi * fo] = rs.uniform(-lim, lim, size=(n_nets, fi * fo)).astype(F32)
        off += fi * fo + fo
    return th


def default_net_map(count: int, n_scenarios: int, n_agents: int) -> np.ndarray:
    """The map agent -> network of a policy set of ``count`` networks when none is given
    (p2pmg_dqn_set_policy_nets with net_of = NULL): int32 [S * N], a % count (role i of every scenario) when
    count == N, the identity when count == S * N, all 0 when count == 1; anything else raises.  Pure NumPy."""
    A = int(n_scenarios) * int(n_agents)
    if count == n_agents:
        return (np.arange(A) % count).astype(np.int32)
    if count == A:
        return np.arange(A, dtype=np.int32)
    if count == 1:
        return np.zeros(A, np.int32)
    raise ValueError(f"a policy set of {count} networks needs net_of: the default maps are for N = {n_agents}, "
                     f"A = {A} or 1 networks")


class DeviceDQNBatch(DeviceCommunityBatch):
    """Device-resident batch of S communities of DQN agents.  All compute runs in libp2pmg.so."""

    def __init__(self, n_scenarios: int, n_agents: int, rounds: int, horizon: int, shared=False,
                 device: int = 0, seed: int = 42, scenario_offset: int = 0, gamma: float = 0.95, tau: float = 0.005,
                 lr: float = 1e-5, capacity: int = 5000, agents_per_block: int = 0, grad_segments: int = 1,
                 init_seed: Optional[int] = 0, **overrides):
        """shared: False (a network per agent of every scenario), True (one network for all) or "role": N
        networks, agent i of every scenario on network i (p2pmg_dqn_setup_roles) -- one community of N
        DQNAgents (agent.py:301-311) trained over S days, weather draws or exploration streams at once."""
        role = isinstance(shared, str)
        if role and shared != "role":
            raise ValueError(f"shared must be False, True or 'role', got {shared!r}")
        super().__init__(n_scenarios, n_agents, rounds, horizon, q_dtype="f32", device=device, seed=seed,
                         scenario_offset=scenario_offset, shared_q=bool(shared), learner=_lib.LEARNER_DQN, **overrides)
        dc = _lib.DqnConfig()
        _lib.check(self.L.p2pmg_dqn_config_default(C.byref(dc)), what="dqn_config_default")
        dc.gamma, dc.tau, dc.lr, dc.capacity, dc.agents_per_block = gamma, tau, lr, capacity, agents_per_block
        dc.grad_segments = grad_segments
        if role:
            self._chk(self.L.p2pmg_dqn_setup_roles(self._ctx, C.byref(dc)), "dqn_setup_roles")
        else:
            self._chk(self.L.p2pmg_dqn_setup(self._ctx, C.byref(dc)), "dqn_setup")
        self.dcfg = dc
        self.shared = "role" if role else bool(shared)
        self.n_nets = self.N if role else (1 if shared else self.A)
        self.capacity = capacity
        self._xfn = None          # the host exchange's ctypes callback (kept alive while installed)
        self._xerr = None
        if init_seed is not None:
            th = glorot_init(self.n_nets, init_seed)
            self.set_weights("online", th)
            self.set_weights("target", th)

    # ----------------------------------------------------------------- networks
    def set_weights(self, which: str, arr, first: int = 0):
        a = np.ascontiguousarray(np.asarray(arr, dtype=F32).reshape(-1, N_PARAMS))
        self._chk(self.L.p2pmg_dqn_set_weights(self._ctx, WHICH[which], first, a.shape[0], a.ctypes.data),
                  f"dqn_set_weights({which})")

    def get_weights(self, which: str, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        count = self.n_nets - first if count is None else count
        out = np.empty((count, N_PARAMS), F32)
        self._chk(self.L.p2pmg_dqn_get_weights(self._ctx, WHICH[which], first, count, out.ctypes.data),
                  f"dqn_get_weights({which})")
        return out

    def initialize_target(self):
        """Trainer.initialize_target (rl.py:274-278): target <- online (soft update with tau = 1)."""
        self.set_weights("target", self.get_weights("online"))

    @property
    def step(self) -> int:
        v = C.c_int64(0)
        self._chk(self.L.p2pmg_dqn_get_step(self._ctx, C.byref(v)), "dqn_get_step")
        return int(v.value)

    @step.setter
    def step(self, value: int):
        self._chk(self.L.p2pmg_dqn_set_step(self._ctx, int(value)), "dqn_set_step")

    def net_steps(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """Adam iterations of each network (one optimizer per DQNAgent, agent.py:310)."""
        count = self.n_nets - first if count is None else count
        out = np.empty(count, np.int64)
        self._chk(self.L.p2pmg_dqn_get_net_steps(self._ctx, first, count, out.ctypes.data), "dqn_get_net_steps")
        return out

    # ----------------------------------------------------------------- learner constants
    def _net_shape(self):
        if self.shared == "role":
            return (self.N,)  # one row per role's network
        return (1,) if self.shared else (self.S, self.N)

    def set_learning(self, gamma=None, tau=None, lr=None, clip=None, penalty_weight=None):
        """Per-network learner constants: each DQNAgent's own Trainer(gamma, tau, Adam(learning_rate))
        (agent.py:306-311) and gradient clip, and each agent's comfort weight (agent.py:225-232).  gamma,
        tau, lr and clip: scalars or anything that broadcasts to [S, N] (per-agent networks), [1] (the
        shared network) or [N] (shared="role": one row per role); penalty_weight broadcasts to [S, N] in either case.  None leaves that field as it
        is; set_learning() restores the values of the constructor.  Takes effect at the next launch; the
        Adam moments and iteration counts stay (p2pmg_dqn_set_learning)."""
        def cast(x, dt, shape):
            if x is None:
                return None
            x = np.asarray(x, dt)
            try:
                return np.ascontiguousarray(np.broadcast_to(x, shape).reshape(-1))
            except ValueError:
                raise ValueError(f"learning arrays must broadcast to {list(shape)}, got {x.shape}") from None
        rows = [cast(x, np.float64, self._net_shape()) for x in (gamma, tau, lr, clip)]
        rows.append(cast(penalty_weight, F32, (self.S, self.N)))
        self._chk(self.L.p2pmg_dqn_set_learning(self._ctx, *(None if x is None else x.ctypes.data for x in rows)),
                  "dqn_set_learning")

    def get_learning(self) -> Dict[str, np.ndarray]:
        """{"gamma", "tau", "lr", "clip": f64 [S, N] (shared network: [1]), "penalty_weight": f32 [S, N]} in use."""
        rows = [np.empty(self.n_nets, np.float64) for _ in range(4)]
        w = np.empty(self.A, F32)
        self._chk(self.L.p2pmg_dqn_get_learning(self._ctx, *(x.ctypes.data for x in rows), w.ctypes.data),
                  "dqn_get_learning")
        out = {k: x.reshape(self._net_shape()) for k, x in zip(("gamma", "tau", "lr", "clip"), rows)}
        out["penalty_weight"] = w.reshape(self.S, self.N)
        return out

    # ----------------------------------------------------------------- multi-rank shared network
    def grad_layout(self) -> dict:
        """Shared network: gradient segments of this context, agents per train workgroup, train
        workgroups per env step (the summation structure the result depends on)."""
        g, a, b = C.c_int(0), C.c_int(0), C.c_int(0)
        self._chk(self.L.p2pmg_dqn_grad_layout(self._ctx, C.byref(g), C.byref(a), C.byref(b)), "dqn_grad_layout")
        return {"segments": g.value, "agents_per_block": a.value, "blocks": b.value}

    def set_grad_exchange(self, gather, rank: int, world: int):
        """Host exchange of the shared network's gradient segments (no RCCL communicator):
        ``gather(segs)`` gets the [world, floats_per_rank] f32 host array with this rank's row
        filled in and must fill the other rows (an all-gather, e.g. over gloo); called once per
        training env step from inside run_episode.  gather=None removes it."""
        if gather is None:
            self._chk(self.L.p2pmg_dqn_set_exchange(self._ctx, _lib.EXCHANGE_FN(), None, 0, 1), "dqn_set_exchange")
            self._xfn = None
            return

        def cb(_user, ptr, per, rk, nr):
            try:
                segs = np.ctypeslib.as_array(ptr, shape=(nr * per,)).reshape(nr, per)
                gather(segs)
                return 0
            except BaseException as e:  # noqa: BLE001  (re-raised by run_episode)
                self._xerr = e
                return 1

        fn = _lib.EXCHANGE_FN(cb)
        self._chk(self.L.p2pmg_dqn_set_exchange(self._ctx, fn, None, int(rank), int(world)), "dqn_set_exchange")
        self._xfn = fn

    # ----------------------------------------------------------------- replay memory
    def set_samples(self, samples):
        """Replay-mode sample indices: deque indices (0 = oldest) of random.sample(buffer, 32)
        (rl.py:238), [T, S, N, 32] or [T, A, 32]."""
        s = np.ascontiguousarray(np.asarray(samples).reshape(self.T, self.A, 32).astype(np.uint16))
        self._chk(self.L.p2pmg_dqn_set_samples(self._ctx, s.ctypes.data), "dqn_set_samples")

    def get_buffer(self, first: int = 0, count: Optional[int] = None):
        """(ring [count, capacity, 10] f32, added [count] int32) of agents [first, first + count)."""
        count = self.A - first if count is None else count
        buf = np.empty((count, self.capacity, 10), F32)
        added = np.empty(count, np.int32)
        self._chk(self.L.p2pmg_dqn_get_buffer(self._ctx, first, count, buf.ctypes.data, added.ctypes.data),
                  "dqn_get_buffer")
        return buf, added

    def set_buffer(self, buf, added, first: int = 0):
        b = np.ascontiguousarray(np.asarray(buf, F32).reshape(-1, self.capacity, 10))
        a = np.ascontiguousarray(np.asarray(added, np.int32).reshape(-1))
        self._chk(self.L.p2pmg_dqn_set_buffer(self._ctx, first, b.shape[0], b.ctypes.data, a.ctypes.data),
                  "dqn_set_buffer")

    # ----------------------------------------------------------------- the hot path
    def run_episode(self, mode: str = "train", rng: str = "philox", episode: int = 0, epsilon: float = 1.0,
                    record: Sequence[str] = (), philox: str = "auto"):
        """One episode of T steps for every scenario (asynchronous, stream-ordered).  epsilon: one rate, or
        [S] rates, scenario s exploring at epsilon[s] as a launch at that scalar would (Philox train / fill
        episodes only: p2pmg_dqn_run_episode_eps)."""
        mask = 0
        for r in record:
            mask |= _lib.REC[r]
        eps = None
        if np.ndim(epsilon) > 0:
            eps = np.ascontiguousarray(epsilon, dtype=np.float64)
            if eps.shape != (self.S,):
                raise ValueError(f"epsilon must be a float or [{self.S}], got {eps.shape}")
            if rng != "philox" or mode not in ("train", "fill"):
                raise ValueError("per-scenario epsilon needs rng='philox' and mode 'train' or 'fill'")
        args = _lib.EpisodeArgs(MODES[mode], _lib.RNG_REPLAY if rng == "replay" else _lib.RNG_PHILOX,
                                int(episode), mask, float(epsilon if eps is None else eps[0]), 0, 0)
        self._xerr = None
        if eps is None:
            st = self.L.p2pmg_run_episode(self._ctx, C.byref(args))
        else:
            st = self.L.p2pmg_dqn_run_episode_eps(self._ctx, C.byref(args), eps)
        if st != _lib.P2PMG_OK and self._xerr is not None:
            raise _lib.P2PMGError(f"run_episode: the gradient exchange raised {self._xerr!r}") from self._xerr
        self._chk(st, "run_episode")
        self._recorded = mask

    # ----------------------------------------------------------------- evaluation
    def set_policy_nets(self, weights, net_of=None):
        """The evaluation policy set: M frozen networks [M, 4609] and the map agent -> network [A] (or
        [S, N]), held on the device beside the learner's arrays and read by run_greedy("policy") alone.
        net_of=None: default_net_map (role a % N for M == N, the identity for M == A, all 0 for M == 1).
        ``weights=None`` (or no rows) drops the set.  A map value outside [0, M) raises and changes nothing."""
        if weights is None or np.size(weights) == 0:
            self._chk(self.L.p2pmg_dqn_set_policy_nets(self._ctx, 0, None, None), "dqn_set_policy_nets")
            return
        w = np.ascontiguousarray(np.asarray(weights, dtype=F32).reshape(-1, N_PARAMS))
        m = default_net_map(w.shape[0], self.S, self.N) if net_of is None else \
            np.ascontiguousarray(np.asarray(net_of).reshape(-1).astype(np.int32))
        if m.size != self.A:
            raise ValueError(f"net_of needs one entry per agent ({self.A}), got {m.size}")
        self._chk(self.L.p2pmg_dqn_set_policy_nets(self._ctx, w.shape[0], w.ctypes.data, m.ctypes.data),
                  "dqn_set_policy_nets")

    def policy_nets(self):
        """(weights [M, 4609] f32, net_of [A] int32) of the policy set in use; None without one."""
        n = C.c_int(0)
        self._chk(self.L.p2pmg_dqn_get_policy_nets(self._ctx, C.byref(n), None, None), "dqn_get_policy_nets")
        if n.value == 0:
            return None
        w = np.empty((n.value, N_PARAMS), F32)
        m = np.empty(self.A, np.int32)
        self._chk(self.L.p2pmg_dqn_get_policy_nets(self._ctx, C.byref(n), w.ctypes.data, m.ctypes.data),
                  "dqn_get_policy_nets")
        return w, m

    def run_greedy(self, source: str = "online", record: Sequence[str] = ()):
        """One greedy episode of T steps for every scenario in ONE launch (dqn_greedy_episode_kernel), on
        the frozen networks of ``source``: "online" or "target" (this batch's own) or "policy" (the policy
        set).  Bit for bit run_episode("greedy") on a per-agent batch holding the mapped networks; trains
        and draws nothing, leaves the learner's state alone (asynchronous, stream-ordered)."""
        if source not in EVAL_SOURCES:
            raise ValueError(f"source must be one of {sorted(EVAL_SOURCES)}, not {source!r}")
        mask = 0
        for r in record:
            mask |= _lib.REC[r]
        self._chk(self.L.p2pmg_dqn_run_greedy(self._ctx, EVAL_SOURCES[source], mask), "dqn_run_greedy")
        self._recorded = mask

    # ----------------------------------------------------------------- object-API primitives
    def forward(self, x, net: int = 0) -> np.ndarray:
        """QNetwork.call (rl.py:147-148) on rows x = concat(state, action) [n, 5]."""
        x = np.ascontiguousarray(np.asarray(x, F32).reshape(-1, 5))
        q = np.empty(x.shape[0], F32)
        self._chk(self.L.p2pmg_dqn_forward(self._ctx, net, x.shape[0], x.ctypes.data, q.ctypes.data), "dqn_forward")
        return q

    def q_values(self, obs, net: int = 0) -> np.ndarray:
        """Q(obs, a) for the three action values (ActorModel.greedy_action rl.py:188-193): [n, 3]."""
        obs = np.asarray(obs, F32).reshape(-1, 4)
        x = np.concatenate([np.repeat(obs, 3, axis=0), np.tile(ACTION_VALUES, len(obs))[:, None]], axis=1)
        return self.forward(x, net).reshape(-1, 3)

    # ----------------------------------------------------------------- the policy map
    def _map_range(self, first: int, count: Optional[int], which: str):
        """(which code, first, count) of a map call, checked before any device call."""
        if which not in MAP_WHICH:
            raise ValueError(f"which must be 'online' or 'target', not {which!r}")
        first = int(first)
        count = self.n_nets - first if count is None else int(count)
        if first < 0 or count < 0 or first + count > self.n_nets:
            raise ValueError(f"networks [{first}, {first + count}) outside [0, {self.n_nets})")
        return MAP_WHICH[which], first, count

    def set_policy_grid(self, time=None, temp=None, balance=None, p2p=None):
        """The grid of observations of the map calls: four f32 axes, state order (time, temp, balance,
        p2p), time slowest.  No axis: back to the default, the table shape at its bins' centres.  A new
        grid drops the map_mark() snapshot."""
        axes = (time, temp, balance, p2p)
        if all(a is None for a in axes):
            self._chk(self.L.p2pmg_dqn_set_grid(self._ctx, None, None, None, None, None), "dqn_set_grid")
            return
        if any(a is None for a in axes):
            raise ValueError("set_policy_grid: give all four axes, or none for the default grid")
        ax = [np.ascontiguousarray(np.asarray(a, F32).reshape(-1)) for a in axes]
        if any(a.size == 0 for a in ax):
            raise ValueError("set_policy_grid: every axis needs at least one value")
        if int(np.prod([a.size for a in ax], dtype=object)) > 2 ** 31 - 1:
            raise ValueError("set_policy_grid: more than 2^31 - 1 grid states")
        n = np.array([a.size for a in ax], np.int32)
        self._chk(self.L.p2pmg_dqn_set_grid(self._ctx, n.ctypes.data, *[a.ctypes.data for a in ax]), "dqn_set_grid")

    def policy_grid(self):
        """The axes in use: (time, temp, balance, p2p) f32 arrays."""
        n = np.zeros(4, np.int32)
        self._chk(self.L.p2pmg_dqn_get_grid(self._ctx, n.ctypes.data, None), "dqn_get_grid")
        ax = np.empty(int(n.sum()), F32)
        self._chk(self.L.p2pmg_dqn_get_grid(self._ctx, n.ctypes.data, ax.ctypes.data), "dqn_get_grid")
        return tuple(np.split(ax, np.cumsum(n)[:-1]))

    def _grid_shape(self):
        n = np.zeros(4, np.int32)
        self._chk(self.L.p2pmg_dqn_get_grid(self._ctx, n.ctypes.data, None), "dqn_get_grid")
        return tuple(int(k) for k in n)

    def policy_map(self, first: int = 0, count: Optional[int] = None, which: str = "online", q: bool = False):
        """The greedy action (0, 1, 2: first maximum) of networks [first, first + count) at every state of
        the grid, evaluated on the device: u8 [count, n0, n1, n2, n3]; q=True: (policy, Q values f32
        [count, n0, n1, n2, n3, 3]), the act kernels' bits."""
        w, first, count = self._map_range(first, count, which)
        shape = self._grid_shape()
        pol = np.empty((count, *shape), np.uint8)
        qv = np.empty((count, *shape, 3), F32) if q else None
        self._chk(self.L.p2pmg_dqn_policy_map(self._ctx, w, first, count, pol.ctypes.data,
                                              qv.ctypes.data if q else None), "dqn_policy_map")
        return (pol, qv) if q else pol

    def map_stats(self, first: int = 0, count: Optional[int] = None, which: str = "online") -> dict:
        """Per network over the grid: {"states": i64 [count], "q_min", "q_max", "abs_max", "min_gap": f64
        [count], "greedy": i64 [count, 3]} (p2pmg_dqn_map_stats)."""
        w, first, count = self._map_range(first, count, which)
        st = np.zeros((count, _lib.DQN_MAP_STATS), np.float64)
        self._chk(self.L.p2pmg_dqn_map_stats(self._ctx, w, first, count, st.ctypes.data), "dqn_map_stats")
        return {"states": st[:, 0].astype(np.int64), "q_min": st[:, 1].copy(), "q_max": st[:, 2].copy(),
                "abs_max": st[:, 3].copy(), "greedy": st[:, 4:7].astype(np.int64), "min_gap": st[:, 7].copy()}

    def map_mark(self, which: str = "online"):
        """Snapshot the packed map of every network of ``which`` on the device (p2pmg_dqn_policy_mark)."""
        w, _, _ = self._map_range(0, 0, which)
        self._chk(self.L.p2pmg_dqn_policy_mark(self._ctx, w), "dqn_policy_mark")

    def map_changes(self, first: int = 0, count: Optional[int] = None, which: str = "online",
                    remark: bool = True) -> np.ndarray:
        """i64 [count]: states whose greedy action differs from the snapshot's; remark=True rewrites the
        snapshot of exactly these networks in the same pass."""
        w, first, count = self._map_range(first, count, which)
        out = np.zeros(count, np.int64)
        self._chk(self.L.p2pmg_dqn_policy_changes(self._ctx, w, first, count, out.ctypes.data, 1 if remark else 0),
                  "dqn_policy_changes")
        return out

    def train_batch(self, s, a, r, ns, net: int = 0) -> float:
        """Trainer._train + update_targets (rl.py:307-359) on one batch of 32 transitions."""
        b = np.concatenate([np.asarray(s, F32).reshape(32, 4), np.asarray(a, F32).reshape(32, 1),
                            np.asarray(r, F32).reshape(32, 1), np.asarray(ns, F32).reshape(32, 4)], axis=1)
        b = np.ascontiguousarray(b)
        loss = C.c_float(0)
        self._chk(self.L.p2pmg_dqn_train_batch(self._ctx, net, b.ctypes.data, C.byref(loss)), "dqn_train_batch")
        return float(loss.value)
